"""The streaming half of gft_kernels.hip at its switch points: axis sums (shift_down), verdict scans (extract_linear, ==,
the zero-pattern query behind the no-zero proofs), padded add / sub / add_scaled and the gather family, on shapes derived
from the dispatch conditions.  Each case names the condition it selects as file:line (genfer_amd/csrc).

Tolerances, no other: exact (integer data against int64 arithmetic; reference-order kernels against the oracle, bit for
bit), conftest.REL_TOL against the oracle (the wave-shuffle sum on positive data), and the order-independent
m u S / (1 - m u) bound against math.fsum (cancelling data) — see _streaming_cases.py.

What no public entry point reaches with a caller-controlled tensor:
  * `is_zero` / `is_constant` never scan (a tensor of more than one coefficient is neither: mt:68-70, 643-645); they are
    checked against the oracle for what they are.
  * `k_any_zero` / `k_zero_pattern` are consulted by `nz_query` (gft_ops_observe.inc:264) from the proven Horner loop of
    an interval `subst_var` (gft_ops_horner.inc:164) only; the tests go through that.  `k_any_zero` needs a tensor with
    more than six non-unit axes (gft_ops_observe.inc:274); one such case is included.  After a "has zeros" answer the
    query backs off (the next 16+ candidates go unasked, :326-328), so WHICH of the cases below launch a scan depends on
    their order; their results must be right either way.
  * the 16-byte alignment terms of the f64x2 selections (gft_kernels.hip:431, 547, 1648) cannot be straddled: every buffer
    comes from the pool, which is aligned.
"""
import contextlib

import numpy as np
import pytest

import _streaming_cases as sc
from conftest import REL_TOL

pytestmark = pytest.mark.gpu


def lib():
    import genfer_amd

    return genfer_amd.lib()


@contextlib.contextmanager
def option(name, value, restore):
    assert lib().gft_set_option(name, float(value)) == 0
    try:
        yield
    finally:
        assert lib().gft_set_option(name, float(restore)) == 0


def same_meta(o, g, what=""):
    assert g.degrees_p1() == o.degrees_p1(), what
    assert g.coeffs_shape() == o.coeffs_shape(), what


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def check_exact(o, g, what=""):
    same_meta(o, g, what)
    a, b = o.array(), g.array()
    if not bit_equal(a, b):
        bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
        raise AssertionError(f"{what}: not bit-exact at {bad[:4].tolist()} of {a.shape}: oracle {a[tuple(bad[0])]!r}, hip {b[tuple(bad[0])]!r}")


# =============================================================================================================================
# 1. axis sums through shift_down
# =============================================================================================================================
def check_shift_down(OTP, GTP, OTPI, GTPI, case, kinds=("int", "pos", "cancel"), host=False, interval=True):
    cid, shape, deg, v, n, order = case
    if host:
        order = "ref"  # the host tier has no wave kernel: HK::sum_axis is the reference's order everywhere
    for seed, kind in enumerate(kinds):
        x = sc.DATA[kind](shape, 7000 + 13 * seed + sum(shape))
        o, g = OTP.new(x, deg).shift_down(v, n), GTP.new(x, deg).shift_down(v, n)
        same_meta(o, g, cid)
        want, got = np.asarray(o.array()), np.asarray(g.array())
        who = f"{cid} [{kind}{', host tier' if host else ''}]"
        if kind == "int":
            exact = sc.shift_down_exact(x, v, n).astype(np.float64)
            assert np.array_equal(got, exact), f"{who}: not the exact integer sum at {np.argwhere(got != exact)[:4].tolist()}"
            assert np.array_equal(want, exact), f"{who}: the ORACLE is not the exact integer sum"
        elif kind == "pos":
            if order == "ref":
                assert bit_equal(got, want), f"{who}: a reference-order kernel differs from the oracle"
            else:
                err = np.abs(got - want)
                print(f"{who}: max rel err vs oracle {np.max(err / np.abs(want)):.3e}")
                assert np.all(err <= REL_TOL * np.abs(want)), who
        else:
            wg = sc.assert_within_fsum_bound(x, v, n, got, f"hip {who}")
            wo = sc.assert_within_fsum_bound(x, v, n, want, f"oracle {who}")
            print(f"{who}: |err| / bound vs fsum: hip {wg:.3e}, oracle {wo:.3e}")
            if order == "ref":
                assert bit_equal(got, want), f"{who}: a reference-order kernel differs from the oracle"
        if not interval:
            continue
        # intervals (always k_sum_axis_seq<EIv>, with the fold where the reference folds): bit for bit, and on integer
        # data an enclosure of the exact sum
        xi = sc.as_interval(x, point=(kind == "int"))
        oi, gi = OTPI.new(xi, deg).shift_down(v, n), GTPI.new(xi, deg).shift_down(v, n)
        check_exact(oi, gi, f"{who} interval")
        if kind == "int":
            iv = np.asarray(gi.array())
            assert np.all(iv[0] <= exact) and np.all(exact <= iv[1]), f"{who}: the interval sum does not enclose the exact sum"


@pytest.mark.parametrize("L", sc.WAVE_LENGTHS)
def test_wave_sum_row_lengths_and_counts(L, OTP, GTP, OTPI, GTPI):
    """k_sum_last_axis_wave (gft_kernels.hip:1597) for L >= 128, the fold for L = 127: rows 1, 3, 4, 5 (a partial block of
    waves), lane loop with partial last trips (129, 191, 193, 1000, 4097)."""
    for case in sc.wave_cases(L):
        check_shift_down(OTP, GTP, OTPI, GTPI, case)


@pytest.mark.parametrize("case", sc.WAVE_EXTRA, ids=[c[0] for c in sc.WAVE_EXTRA])
def test_wave_sum_prefixes_rank3_and_second_row_trip(case, OTP, GTP, OTPI, GTPI):
    check_shift_down(OTP, GTP, OTPI, GTPI, case, interval=sc.numel(case[1]) <= 1 << 16)


@pytest.mark.parametrize("L", sc.UNROLL8_LENGTHS + (128, 200))
def test_fold_of_eight_bit_exact(L, OTP, GTP, OTPI, GTPI):
    """SUM_UNROLL8 (gft_kernels.hip:1573-1586): main loop, tail, and the combine order, f64 and interval.  L = 128, 200:
    f64 is on the wave kernel there, the interval twin still folds."""
    for case in sc.unroll8_cases(L):
        if L >= 128:  # inner == 1 && upto >= 128 (gft_ops_observe.inc:448) holds for v = 0 with shape[1] == 1 as well
            case = case[:5] + ("wave",)
        check_shift_down(OTP, GTP, OTPI, GTPI, case)


def test_slab_by_slab_sums_bit_exact(OTP, GTP, OTPI, GTPI):
    """k_sum_axis_seq / k_sum_axis_seq_f64x2 on either side of gft_kernels.hip:1647 (inner even / odd, odd stride)."""
    for case in sc.seq_cases():
        check_shift_down(OTP, GTP, OTPI, GTPI, case)


@pytest.mark.parametrize("case", sc.BIG_SEQ_CASES, ids=[c[0] for c in sc.BIG_SEQ_CASES])
def test_slab_by_slab_sums_above_one_grid_pass(case, OTP, GTP, OTPI, GTPI):
    check_shift_down(OTP, GTP, OTPI, GTPI, case, kinds=("int", "pos"), interval=False)


def test_interval_sum_above_one_grid_pass(OTP, GTP, OTPI, GTPI):
    check_shift_down(OTP, GTP, OTPI, GTPI, sc.BIG_INTERVAL_CASE, kinds=("int",))


def test_small_sums_on_the_host_tier(OTP, GTP, OTPI, GTPI):
    """HK::sum_axis (gft_host.hpp:300): the same cases with the tensors on the host tier — every order is the reference's."""
    import genfer_amd

    with option(b"host_max_elems", 1 << 17, 0.0):
        before = genfer_amd.op_stats()["host_tier_ops"]
        cases = sc.small_shift_cases()
        for case in cases:
            check_shift_down(OTP, GTP, OTPI, GTPI, case, host=True)
        assert genfer_amd.op_stats()["host_tier_ops"] - before >= 6 * len(cases), "the sums did not run on the host tier"


# =============================================================================================================================
# 2. verdict scans
# =============================================================================================================================
@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("shape,blocks", sc.SCAN_SHAPES, ids=["128-blocks", "1024-blocks"])
def test_linear_scan_spoiler_positions(shape, blocks, interval, OTP, GTP, OTPI, GTPI):
    """k_linear_scan (gft_kernels.hip:1067, block count :1148): a tensor linear in axis 0, then one spoiling coefficient
    where only one of the four clamped loads, only the second trip, or only the last thread sees it.  Scans alternate
    "not linear" / "linear" on one stream, so a state word left behind by one (:1136-1137) would spoil the next."""
    import genfer_amd

    O, G = (OTPI, GTPI) if interval else (OTP, GTP)
    mk = (lambda a: np.stack([a, a])) if interval else (lambda a: a)
    t = sc.linear_tensor(shape)
    clean_o = O.new(mk(t), shape).extract_linear()
    assert clean_o is not None and clean_o[2] == 0
    scans0 = genfer_amd.op_stats()["linear_scans"]
    n_scans = 0
    s = mk(t.copy())
    for pos in sc.spoiler_positions(shape, blocks):
        for plane in range(s.shape[0] if interval else 1):
            tgt = s[plane] if interval else s
            tgt.flat[pos] = 0.5
        want = O.new(s, shape).extract_linear()
        g = G.new(s, shape)
        assert want is None and g.extract_linear() is None, f"spoiler at {pos} of {sc.numel(shape)} went unseen"
        assert g.is_constant() is False
        for plane in range(s.shape[0] if interval else 1):
            tgt = s[plane] if interval else s
            tgt.flat[pos] = 0.0
        assert G.new(s, shape).extract_linear() == clean_o, f"the scan after the spoiler at {pos}"
        n_scans += 2
    assert genfer_amd.op_stats()["linear_scans"] - scans0 == n_scans, "a verdict did not come from the device scan"
    # a coefficient with two non-zero axes; for intervals also [0, tiny] at the very last element (not an exact zero)
    s = t.copy()
    s[(1, 1) + (0,) * (len(shape) - 2)] = 0.5
    assert O.new(mk(s), shape).extract_linear() is None and G.new(mk(s), shape).extract_linear() is None
    if interval:
        s = np.stack([t, t])
        s[1].flat[sc.numel(shape) - 1] = 5e-324
        assert OTPI.new(s, shape).extract_linear() is None and GTPI.new(s, shape).extract_linear() is None
    # linear in the LAST axis, and the constant tensor's verdict
    t2 = np.zeros(shape)
    t2.flat[0], t2.flat[1] = 2.5, -0.125
    assert G.new(mk(t2), shape).extract_linear() == O.new(mk(t2), shape).extract_linear() != None  # noqa: E711


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_equality_single_difference_above_one_grid_pass(interval, OTP, GTP, OTPI, GTPI):
    """k_count_neq (gft_kernels.hip:1661): equal everywhere; one differing element in the first, second, third grid-stride
    trip and at the very end; a NaN (x == x is false, mt:10 derives PartialEq)."""
    O, G = (OTPI, GTPI) if interval else (OTP, GTP)
    mk = (lambda a: np.stack([a, a + 1.0])) if interval else (lambda a: a)
    x = sc.pos_data(sc.EQ_SHAPE, 4242)
    ao, ag = O.new(mk(x), sc.EQ_SHAPE), G.new(mk(x), sc.EQ_SHAPE)
    assert (ao == O.new(mk(x), sc.EQ_SHAPE)) is True and (ag == G.new(mk(x), sc.EQ_SHAPE)) is True
    for pos in sc.EQ_POSITIONS:
        y = x.copy()
        y.flat[pos] = np.nextafter(y.flat[pos], 2.0)
        assert (ao == O.new(mk(y), sc.EQ_SHAPE)) is False and (ag == G.new(mk(y), sc.EQ_SHAPE)) is False, pos
        if interval:  # only the upper endpoint differs
            yi = mk(x)
            yi[1].flat[pos] = np.nextafter(yi[1].flat[pos], 9.0)
            assert (ao == O.new(yi, sc.EQ_SHAPE)) is False and (ag == G.new(yi, sc.EQ_SHAPE)) is False, pos
        y = x.copy()
        y.flat[pos] = np.nan
        bo, bg = O.new(mk(y), sc.EQ_SHAPE), G.new(mk(y), sc.EQ_SHAPE)
        assert (bo == bo) is False and (bg == bg) is False, pos
        assert (ao == bo) is False and (ag == bg) is False, pos
    assert (ag == G.new(mk(x), sc.EQ_SHAPE)) is True  # (the count word is cleared per call: gft_api.hip:1131)


# ---- the zero-pattern query behind the no-zero proofs ----------------------------------------------------------------------------
NZ_SHAPES = [
    ((3, 8192), "zero_pattern"),                 # 24 576 > 64 x 256: k_zero_pattern grid-strides (gft_kernels.hip:1706, :1731)
    ((3, 2, 2, 2, 2, 2, 342), "any_zero"),       # seven non-unit axes -> k_any_zero (gft_ops_observe.inc:274, :321); 32 832 elements
]


def nz_variants(shape):
    x = sc.pos_data(shape, 515)
    base = np.stack([x, x + 0.25])
    yield "no zero", base
    v = base.copy()
    v[0].flat[-1] = v[1].flat[-1] = 0.0
    yield "[0,0] at the last element", v
    v = base.copy()
    v[0].flat[-1], v[1].flat[-1] = 0.0, 5e-324
    yield "[0,tiny] at the last element", v
    v = base.copy()
    v[:, 0] = 0.0
    yield "slab 0 of axis 0 exactly zero", v
    v = base.copy()
    v[..., 0] = 0.0
    yield "slab 0 of the last axis exactly zero", v


def test_zero_queries_do_not_change_a_substitution(OTPI, GTPI):
    """An interval subst_var(0, c + m x_last) with c a non-zero finite interval is a proven Horner loop
    (gft_ops_horner.inc:132-137) and asks where the coefficient tensor's zeros are (:164).  A wrong answer shows only as
    a different computation: the result must be the oracle's bit for bit with nz_proofs on and off.

    Order matters for what is ASKED, not for what must hold: "no zero" and slab answers leave the back-off at rest, an
    irregular zero (and every zero k_any_zero finds) starts it.  So both shapes go first with the zero-free data, then
    k_zero_pattern gets its slabs and the single zero at the last element; the seven-axis tensor's zeros come last and
    may go unasked."""
    variants = {}
    for shape, _ in NZ_SHAPES:
        variants[shape] = dict(nz_variants(shape))
    (zp, _), (az, _) = NZ_SHAPES
    names = list(variants[zp])
    order = [(az, names[0]), (zp, names[0]), (az, names[2]), (zp, names[2]), (zp, names[3]), (zp, names[4]), (zp, names[1]),
             (az, names[3]), (az, names[4]), (az, names[1])]
    for shape, name in order:
        data = variants[shape][name]
        last = len(shape) - 1
        sub = np.zeros((2,) + (1,) * last + (2,))
        sub[0].flat[:], sub[1].flat[:] = (0.5, 0.25), (0.5 + 2 ** -40, 0.25 + 2 ** -40)
        want = OTPI.new(data, shape).subst_var(0, OTPI.new(sub, shape))
        got = {}
        for proofs in (1, 0):
            with option(b"nz_proofs", proofs, 1):
                got[proofs] = GTPI.new(data, shape).subst_var(0, GTPI.new(sub, shape))
                check_exact(want, got[proofs], f"{shape}: {name}, nz_proofs={proofs}")
        assert bit_equal(got[1].array(), got[0].array()), (shape, name)


# =============================================================================================================================
# 3. padded add / sub / add_scaled and the gather switches
# =============================================================================================================================
ADD_CASES = [
    # (id, degrees, stored shape of a, stored shape of b)
    # equal shapes, even total, 526 500 pairs: k_addsub_f64x2's grid-stride second trip (gft_kernels.hip:547-551)
    ("equal-even", (10, 300, 351), (10, 300, 351), (10, 300, 351)),
    # equal shapes, odd total (544 509): (total & 1) fails at :547 -> k_addsub_padded with nothing to pad
    ("equal-odd", (9, 301, 201), (9, 301, 201), (9, 301, 201)),
    # one compact operand (:549)
    ("one-compact", (9, 301, 201), (9, 301, 201), (9, 120, 201)),
    ("one-compact-even", (9, 300, 202), (9, 300, 202), (9, 120, 202)),
    # both compact, on different axes: the result is larger than either (max_shape, gft_ops_core.inc:872)
    ("both-compact", (9, 301, 201), (9, 120, 201), (4, 301, 77)),
]


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("case", ADD_CASES, ids=[c[0] for c in ADD_CASES])
def test_padded_add_sub_add_scaled_above_one_grid_pass(case, interval, OTP, GTP, OTPI, GTPI):
    """k_addsub_padded / k_addsub_f64x2 / k_add_scaled_padded (gft_kernels.hip:467-555) above 524 288 elements."""
    _, deg, sa, sb = case
    O, G = (OTPI, GTPI) if interval else (OTP, GTP)
    mk = sc.as_interval if interval else (lambda a: a)
    xa, xb = mk(sc.cancel_data(sa, 31)), mk(sc.pos_data(sb, 32) - 1.0)
    c = (0.3, 0.3000001) if interval else 0.3
    ao, bo, ag, bg = O.new(xa, deg), O.new(xb, deg), G.new(xa, deg), G.new(xb, deg)
    check_exact(ao + bo, ag + bg, "a + b")
    check_exact(ao - bo, ag - bg, "a - b")
    check_exact(bo - ao, bg - ag, "b - a")
    check_exact(ao.add_scaled(bo, c), ag.add_scaled(bg, c), "a + c b")
    check_exact(bo.add_scaled(ao, c), bg.add_scaled(ag, c), "b + c a")


# K<E>::gather (gft_kernels.hip:428-459).  f64x2 (:430-433): last axis unshifted, even, not the table's axis.  Row kernel
# (:453): last >= 48, total >= 2^20, rows >= 4096.  Otherwise k_gather (grid-strided above 524 288 elements), or k_gather_htab
# for by-value tables (:443).  An operation along axis v of a tensor `shape` gathers into shape - e_v (or shape + e_v).
GATHER_SHAPES = [
    # derivative(0,1) -> (150,150,47): last = 47 < 48 -> k_gather; derivative(2,1) -> last 46, shifted -> k_gather
    ("last47", (151, 150, 47)),
    # derivative(0,1) -> (148,148,48): even, unshifted -> k_gather_f64x2; derivative(2,1) on last 49 -> 48, shifted -> rows
    ("last48-49", (149, 148, 49)),
    # rank 2, rows = 4095 < 4096 -> k_gather at total 1 052 415 >= 2^20 (odd last: no f64x2)
    ("rows4095", (4095, 257)),
    # rows = 4097 -> k_gather_rows; derivative(1,1) -> last 256 even but shifted -> rows; truncation -> f64x2
    ("rows4097", (4097, 257)),
    # rows = 4100, last = 255: total 1 045 500 < 2^20 -> k_gather ...
    ("below-2^20", (4100, 255)),
    # ... and last = 256: 1 049 600 >= 2^20; unshifted even -> f64x2, shifted (derivative along the last axis) -> rows
    ("above-2^20-even", (4100, 256)),
]


def gather_results(T, p, shape, sv):
    """(name, result) of every gather-backed operation, along the leading and the last axis."""
    nd = len(shape)
    for v in (0, nd - 1):
        yield f"derivative({v},1)", p.derivative(v, 1)               # OP_MUL_TAB, tab_axis = v (== last or not)
        yield f"derivative({v},2)", p.derivative(v, 2)
        yield f"taylor_expansion_of_coeff({v},1)", p.taylor_expansion_of_coeff(v, 1)
        yield f"coefficients_of_term({v},1)", p.coefficients_of_term(v, 1)
        yield f"taylor_polynomial_terms({v},[0,2])", p.taylor_polynomial_terms(v, [0, 2])  # keep-mask
        yield f"* var({v},0)", p * T.var(v, sv(0.0), shape[v])     # shift -1 along v
        lin = np.zeros(tuple(2 if ax == v else 1 for ax in range(nd)))
        lin.flat[1] = 0.75
        if T.WIDTH == 2:
            lin = np.stack([lin, lin * (1.0 + 2.0 ** -30)])
        yield f"subst_var({v}, 0.75 x)", p.subst_var(v, T.new(lin, list(shape)))  # scanned subst: m known on the host
        m = (0.9048374180359595, 0.9048374180359597) if T.WIDTH == 2 else 0.9048374180359595
        yield f"subst_var({v}, var * m)", p.subst_var(v, T.var(v, sv(0.0), shape[v]) * T.from_scalar(m))
    yield "truncate_to_degree_p1", p.truncate_to_degree_p1(min(shape) - 3)
    yield "extend", p.extend([s + 1 for s in shape])


@pytest.mark.parametrize("defer", [1, 0], ids=["deferred", "launched"])
@pytest.mark.parametrize("name,shape", GATHER_SHAPES, ids=[n for n, _ in GATHER_SHAPES])
def test_gather_switches_bit_exact(name, shape, defer, OTP, GTP):
    """Every gather-backed operation on either side of each condition of K<E>::gather.  With `defer` on, elementwise
    results are chain stages that the consuming array() materialises; with it off every operation is its own gather
    launch (scaled substitutions then take OP_MUL_HTAB up to 384 powers, an uploaded OP_MUL_TAB above)."""
    x = sc.pos_data(shape, 1701) - 0.75
    with option(b"defer", defer, 1):
        o, g = OTP.new(x, list(shape)), GTP.new(x, list(shape))
        for (what, ro), (_, rg) in zip(gather_results(OTP, o, shape, float), gather_results(GTP, g, shape, float)):
            check_exact(ro, rg, f"{name} {shape}: {what}")


@pytest.mark.parametrize("defer", [1, 0], ids=["deferred", "launched"])
@pytest.mark.parametrize("name,shape", [GATHER_SHAPES[1], GATHER_SHAPES[3]], ids=[GATHER_SHAPES[1][0], GATHER_SHAPES[3][0]])
def test_gather_switches_interval_bit_exact(name, shape, defer, OTPI, GTPI):
    """Interval tensors never take the f64x2 path: the row kernel above the thresholds, k_gather / k_gather_htab below."""
    x = sc.pos_data(shape, 1702) - 0.75
    xi = sc.as_interval(x)
    with option(b"defer", defer, 1):
        o, g = OTPI.new(xi, list(shape)), GTPI.new(xi, list(shape))
        iv = lambda s: (s, s)  # noqa: E731
        for (what, ro), (_, rg) in zip(gather_results(OTPI, o, shape, iv), gather_results(GTPI, g, shape, iv)):
            check_exact(ro, rg, f"{name} {shape}: {what}")
