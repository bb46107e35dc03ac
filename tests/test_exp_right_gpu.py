"""The right-looking tiled exponential (exp_rec, gft_ops_recur.inc) of rank >= 3 at the edges of its host loop, against an
exact rational reference.

The path is the default of every f64 exp of rank >= 3 with total >= 64 * tiled_min_macs; lowering the run-time option
tiled_min_macs lets it run at shapes small enough for fractions.Fraction (_exp_exact.py; the cases are its CASES table,
the CPU twin test_exp_right_cpu.py holds the oracle to the same bound on each of them).  The tolerance is the project's
contract and nothing tighter:  |got - seed * E| <= 1e-10 * seed * M  per coefficient, E the exact exponential of a - c0, M
that of |a - c0| (non-negative arguments: M = E, 1e-10 relative), seed = got[0, .., 0] checked separately against libm's
exp(c0) to 4 ulp, so that libm stays out of the bound.  Every case asserts through op_stats that its steps ran on the
tiled kernel.

Measured worst ratio |got - exact| / M over all cases: see WORST_MEASURED below (the oracle's own: 9.4e-16)."""
import contextlib
import math
from fractions import Fraction

import numpy as np
import pytest

from _exp_exact import CASES, case_data, case_reference, result_shape, worst_ratio

CONTRACT = Fraction(1, 10 ** 10)
LOWERED = 1.0  # tiled_min_macs during the small cases: every step product is "large"
WORST_MEASURED = "GPU 1.4e-15 (full_inner32, positive), oracle 9.4e-16 (last_over_128, positive)"


@contextlib.contextmanager
def options(**opts):
    """gft_set_option for the block; the project's defaults afterwards."""
    import genfer_amd

    defaults = {"tiled_min_macs": 2.0e5, "exp_right": 1.0}
    L = genfer_amd.lib()
    try:
        for k, v in opts.items():
            assert L.gft_set_option(k.encode(), float(v)) == 0
        yield
    finally:
        for k in opts:
            assert L.gft_set_option(k.encode(), defaults[k]) == 0


def _stats_delta(before, after):
    return {k: after[k] - before[k] for k in ("tiled", "staged", "per_output", "host_tier_ops")}


def _bit_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def _check_exact(name, positive, got):
    deg, xs, _ = CASES[name]
    a, c0, E, M = case_reference(name, positive)
    assert got.shape == result_shape(deg, xs), (got.shape, result_shape(deg, xs))
    seed = got[(0,) * got.ndim]
    assert abs(seed - math.exp(c0)) <= 4 * math.ulp(math.exp(c0))
    ratio = worst_ratio(got, E, M, seed)
    print(f"gpu {name} {'positive' if positive else 'mixed'}: worst ratio {float(ratio):.3e}")
    assert ratio <= CONTRACT, (name, float(ratio))


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["device", "host"], indirect=True)
@pytest.mark.parametrize("positive", [False, True], ids=["mixed", "positive"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_right_looking_exp_against_the_exact_series(name, positive, tier, OTP, GTP):
    """Every case of _exp_exact.CASES with tiled_min_macs lowered: the contract against the exact series, and (device tier)
    `tiled` rises by exactly the case's number of steps with work.  rank5: its one rank-5 step of two slabs is refused by
    conv_tiled_high_rank (accumulate) and by the planner (rank 5), so it runs on the reference-order kernel (`staged` /
    `per_output` rises); the one-slab steps collapse to rank 4 and lower and are tiled.  On the host tier the small cases
    run on the host (no right-looking form there): those are bit-identical to the oracle."""
    import genfer_amd

    deg, xs, steps = CASES[name]
    a = case_data(name, positive)
    with options(tiled_min_macs=LOWERED):
        before = genfer_amd.op_stats()
        got = np.asarray(GTP.new(a, list(deg)).exp().array())
        delta = _stats_delta(before, genfer_amd.op_stats())
    print(name, tier, delta)
    _check_exact(name, positive, got)
    if tier == "device":
        assert delta["tiled"] == steps, delta
        if name == "rank5":
            assert delta["staged"] + delta["per_output"] >= 1, delta
    elif delta["tiled"] == 0 and delta["host_tier_ops"] > 0:
        assert _bit_equal(got, OTP.new(a, list(deg)).exp().array())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_left_looking_exp_stays_in_reference_order(name, OTP, GTP):
    """The same cases with exp_right 0.  Where the row wavefront takes the recurrence the result is bit-identical to the
    oracle; where it declines (rows longer than 64 at rank 3, a unit axis, fewer than 8 rows, rank 5) the slab steps are
    products of shifted operand views, tiled under the lowered threshold — six of the cases, which thereby cover that form
    at exactly checkable shapes: the contract against the exact series."""
    import genfer_amd

    deg, xs, _ = CASES[name]
    a = case_data(name)
    with options(tiled_min_macs=LOWERED, exp_right=0):
        before = genfer_amd.op_stats()
        got = np.asarray(GTP.new(a, list(deg)).exp().array())
        delta = _stats_delta(before, genfer_amd.op_stats())
    print(name, "exp_right=0", delta)
    if delta["tiled"] == 0:
        assert _bit_equal(got, OTP.new(a, list(deg)).exp().array())
    else:
        assert name in ("last_over_128", "unit_middle", "unit_last", "full_inner28", "full_inner16", "rank5"), (name, delta)
        _check_exact(name, False, got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["full_inner28", "compact_mid_last", "last_over_128", "rank4"])
def test_interval_exp_ignores_the_options(name, OTPI, GTPI):
    """Intervals have no right-looking form (W == 1 is part of its condition): bit-exact against the oracle with the
    threshold lowered, and no tiled product."""
    import genfer_amd

    deg, xs, _ = CASES[name]
    a = case_data(name)
    ai = np.stack([a, a + np.abs(a) * 2.0 ** -30])
    with options(tiled_min_macs=LOWERED):
        before = genfer_amd.op_stats()
        got = GTPI.new(ai, list(deg)).exp().array()
        delta = _stats_delta(before, genfer_amd.op_stats())
    assert delta["tiled"] == 0, delta
    assert _bit_equal(got, OTPI.new(ai, list(deg)).exp().array())


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
def test_right_looking_exp_with_a_non_finite_coefficient(bad, OTP, GTP):
    """One inf / NaN at an interior position of the operand: the guarded fallback runs in ACCUMULATE mode here (the steps
    add into slabs of the result).  The non-finite pattern equals the oracle's exactly; the finite coefficients (those no
    term of which meets the bad one) meet the contract against the oracle, the majorant taken on |a| without the bad
    coefficient; and a following finite exp on the same stream is unaffected (the guard stamp is per product)."""
    import genfer_amd

    name = "lead3_under_6"
    deg, xs, steps = CASES[name]
    a = case_data(name)
    a[1, 3, 4] = bad
    clean = np.abs(a)
    clean[1, 3, 4] = 0.0
    with options(tiled_min_macs=LOWERED):
        before = genfer_amd.op_stats()
        got = np.asarray(GTP.new(a, list(deg)).exp().array())
        delta = _stats_delta(before, genfer_amd.op_stats())
        after_bad = np.asarray(GTP.new(case_data(name), list(deg)).exp().array())
    assert delta["tiled"] == steps, delta
    want = np.asarray(OTP.new(a, list(deg)).exp().array())
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
    fin = np.isfinite(want)
    assert fin.any() and not fin.all()
    M = np.asarray(OTP.new(clean, list(deg)).exp().array())
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-10 * M[fin])
    _check_exact(name, False, after_bad)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,tiled_steps", [((22, 22, 22), 15), ((24, 20, 32), 20)], ids=["22cubed", "24x20x32"])
def test_right_looking_exp_at_the_real_crossover(shape, tiled_steps, OTP, GTP):
    """No option touched: 22^3 is the smallest full cube with total = (n^2 / 2 + 1/2)^3 >= 64 * 2e5 (21^3: 1.08e7, 22^3:
    1.43e7), (24, 20, 32) has rows of whole chunks.  Auto mode takes the right-looking path by itself; of its n0 - 1 steps
    those of m slabs with m / 2 * (n1^2 / 2) (n2^2 / 2) >= 2e5 multiply-adds (m >= 7 resp. m >= 4) run on the tiled kernel,
    the short ones at the end on the reference-order kernel.  Against the oracle under the contract (majorant: the oracle's
    exp of |a|)."""
    import genfer_amd

    from conftest import splitmix64_uniform

    a = (-0.2 + 0.4 * splitmix64_uniform(4242 + shape[0], int(np.prod(shape)))).reshape(shape)
    before = genfer_amd.op_stats()
    got = np.asarray(GTP.new(a, list(shape)).exp().array())
    delta = _stats_delta(before, genfer_amd.op_stats())
    print(shape, delta)
    assert delta["tiled"] == tiled_steps, delta
    want = np.asarray(OTP.new(a, list(shape)).exp().array())
    M = np.asarray(OTP.new(np.abs(a), list(shape)).exp().array())
    assert np.all(np.abs(got - want) <= 1e-10 * M), np.max(np.abs(got - want) / M)


@pytest.mark.gpu
def test_shifted_view_slab_step_is_still_reachable(OTP, GTP):
    """The left-looking slab step on the tiled kernel (K::conv's shifted operand views, j0_min = 1) is what exp_rec comes to
    when the wavefront declines and the right-looking form is below its crossover: a rank-2 exp of fewer than 8 rows
    (plan_wavefront wants 8) with rows long enough for one slab step to be worth the tiled kernel.  (6, 900): total =
    18.5 * 405000.5 = 7.5e6 < 1.28e7; step k = 5 is 5 * 405000 = 2.03e6 multiply-adds >= 10 * 2e5 (split), step 4 is not."""
    import genfer_amd

    from conftest import splitmix64_uniform

    shape = (6, 900)
    a = (-0.2 + 0.4 * splitmix64_uniform(977, int(np.prod(shape)))).reshape(shape)
    before = genfer_amd.op_stats()
    got = np.asarray(GTP.new(a, list(shape)).exp().array())
    delta = _stats_delta(before, genfer_amd.op_stats())
    print(shape, delta)
    assert delta["tiled"] == 1, delta
    want = np.asarray(OTP.new(a, list(shape)).exp().array())
    M = np.asarray(OTP.new(np.abs(a), list(shape)).exp().array())
    assert np.all(np.abs(got - want) <= 1e-10 * M), np.max(np.abs(got - want) / M)
