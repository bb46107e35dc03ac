"""The division / log / exp kernels of gft_div2d.hip on data that leaves their fast paths in the middle of a computation
(tests/_recur_edge_cases.py: growth past the exponent window to inf and NaN, decay below it to denormals and signed zeros, the
divisor sweep), at the smallest shape that reaches each kernel, with full and compact operands, f64 and intervals: the bit
patterns of every coefficient against the oracle's — the sign of a zero included; a NaN only has to be a NaN.  That the cases
do cross the switches is test_recur_edges_cpu.py's business (on the oracle alone)."""
import numpy as np
import pytest

import _recur_edge_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import genfer_amd

    return genfer_amd.lib()


def launches():
    import genfer_amd

    return genfer_amd.op_stats()["launches"]


def assert_same(what, want, g):
    """`want`: (array, degrees_p1, coeffs_shape) of the oracle; g: the product's polynomial"""
    a, deg, stored = want
    assert g.degrees_p1() == deg, (what, g.degrees_p1(), deg)
    assert g.coeffs_shape() == stored, (what, g.coeffs_shape(), stored)
    got = np.asarray(g.array())
    msg = rc.describe_mismatch(what, a, got)
    assert msg is None, msg
    return got


def number_kinds(row, OTP, GTP, OTPI, GTPI, var=None):
    return [("f64", OTP, GTP, lambda a: a)] + [(f"interval_{k}", OTPI, GTPI, w) for k, w in rc.interval_kinds(row, var)]


def wavefront_settings(row):
    return (1, 0) if row.wf0 else (1,)


@pytest.mark.parametrize("row,fam,ax,var,xs,ys", rc.CASES, ids=rc.CASE_IDS)
def test_division_across_the_switches_bit_exact(row, fam, ax, var, xs, ys, OTP, GTP, OTPI, GTPI, L):
    x, y = rc.operands(row, fam, ax, xs, ys)
    deg = list(row.shape)
    cid = rc.case_id(row, fam, ax, var)
    for kind, O, G, mk in number_kinds(row, OTP, GTP, OTPI, GTPI, var):
        want = rc.oracle_div(O, cid if kind == "f64" else (cid, kind[9:]), mk(x), mk(y), deg)
        got = {}
        for wf in wavefront_settings(row):
            assert L.gft_set_option(b"div_wavefront", float(wf)) == 0
            try:
                before = launches()
                g = G.new(mk(x), deg) / G.new(mk(y), deg)
                got[wf] = assert_same(f"{row.kernel} {cid} {kind} div_wavefront={wf}", want, g)
                if wf and row.one_launch:
                    assert launches() - before <= 8, f"{cid}: the long-row quotient did not take the one-launch wavefront"
            finally:
                L.gft_set_option(b"div_wavefront", 1.0)
        if len(got) == 2:
            msg = rc.describe_mismatch(f"{cid} {kind}: wavefront against the blocked recurrence", got[0], got[1])
            assert msg is None, msg


LOG_ROWS = [r for r in rc.TABLE if r.log]


@pytest.mark.parametrize("row", LOG_ROWS, ids=[r.id for r in LOG_ROWS])
def test_log_across_the_switches_bit_exact(row, OTP, GTP, OTPI, GTPI, L):
    """log's recurrence (a division by xs[0] per slab, then / k) through the fused slab step and the wavefronts' log mode"""
    deg = list(row.shape)
    for name, arg in rc.log_arguments(row):
        for kind, O, G, mk in number_kinds(row, OTP, GTP, OTPI, GTPI):
            want = rc.oracle_unary(O, (row.id, name, kind), "log", mk(arg), deg)
            got = {}
            for wf in wavefront_settings(row):
                assert L.gft_set_option(b"div_wavefront", float(wf)) == 0
                try:
                    got[wf] = assert_same(f"log {row.kernel} {row.id} {name} {kind} div_wavefront={wf}", want, G.new(mk(arg), deg).log())
                finally:
                    L.gft_set_option(b"div_wavefront", 1.0)
            if len(got) == 2:
                msg = rc.describe_mismatch(f"log {row.id} {name} {kind}: wavefront against the blocked recurrence", got[0], got[1])
                assert msg is None, msg


EXP_ROWS = [r for r in rc.TABLE if r.exp]


@pytest.mark.parametrize("row", EXP_ROWS, ids=[r.id for r in EXP_ROWS])
def test_exp_of_decaying_series_bit_exact(row, OTP, GTP, OTPI, GTPI, L):
    """exp in the reference's order (`exp_right` 0, no tiled steps, as test_div_row_wavefront_bit_exact runs it) on the decay
    family; exp's non-finite handling has test_exp_right_gpu.py"""
    deg = list(row.shape)
    arg = rc.decay(row.shape)[1]
    L.gft_set_option(b"exp_right", 0.0)
    L.gft_set_option(b"tiled_min_macs", 1e30)
    try:
        for kind, O, G, mk in number_kinds(row, OTP, GTP, OTPI, GTPI):
            want = rc.oracle_unary(O, (row.id, "decay", kind), "exp", mk(arg), deg)
            for wf in wavefront_settings(row):
                assert L.gft_set_option(b"div_wavefront", float(wf)) == 0
                try:
                    assert_same(f"exp {row.kernel} {row.id} {kind} div_wavefront={wf}", want, G.new(mk(arg), deg).exp())
                finally:
                    L.gft_set_option(b"div_wavefront", 1.0)
    finally:
        L.gft_set_option(b"exp_right", 1.0)
        L.gft_set_option(b"tiled_min_macs", 2e5)


@pytest.mark.parametrize("shape,reduced", rc.SWEEP_SHAPES, ids=["x".join(map(str, s)) for s, _ in rc.SWEEP_SHAPES])
def test_divisor_sweep_every_quotient_correctly_rounded(shape, reduced, OTP, GTP):
    """independent quotients x[c] / d through the kernels' slab division: numpy's correctly rounded x / d for divisors and
    numerators on both sides of every edge of the exponent window, and the oracle's bits for the whole result"""
    for i, d in enumerate(rc.sweep_divisors(reduced)):
        x, y, valid = rc.divisor_sweep(shape, float(d), seed=2501 + 7 * i)
        g = GTP.new(x, list(shape)) / GTP.new(y, list(shape))
        got = np.asarray(g.array())
        assert got.shape == tuple(shape)
        with np.errstate(under="ignore"):
            want = x / d
        msg = rc.describe_mismatch(f"sweep {shape} d = {float(d)!r} ({float(d).hex()})", want[valid], got[valid])
        assert msg is None, msg
        assert_same(f"sweep {shape} d = {float(d)!r} against the oracle", rc.oracle_div(OTP, ("sweep", shape, i), x, y, list(shape)), g)


def test_rows64_row_of_negative_zero_numerators_keeps_its_sign(OTP, GTP):
    """Regression: k_div_2d_rows64 forms every quotient of a row with the three-instruction form and settles afterwards whether
    a numerator was outside its domain.  -0 is outside (q = -0, residual +0, +0 + -0 = +0 instead of IEEE's -0 / d = -0) but
    counted as inside, so a row whose numerators were all -0 — beyond the dividend's last row, with partial sums of +0 — came
    out as +0.  (First seen as 70x24-decay-compact_dividend with `div_wavefront` 0.)"""
    x, y = rc.negative_zero_rows()
    deg = list(y.shape)
    g = GTP.new(x, deg) / GTP.new(y, deg)
    assert_same("k_div_2d_rows64, rows of -0 numerators", rc.oracle_div(OTP, "negative_zero_rows", x, y, deg), g)


# ---- series.div: forms A and B, four items a batch ----------------------------------------------------------------------------------


def series_batch(n):
    """items in order: benign, growth, decay, one inf in the middle of the dividend"""
    bx, by = rc.rand((n,), 2601, -1.0, 1.0), rc.rand((n,), 2602, -0.2, 0.2)
    by[0] = 1.5
    gx, gy = rc.growth((n,), 0)
    dx, dy = rc.decay((n,))
    ix = bx.copy()
    ix[n // 2] = np.inf
    return np.stack([bx, gx, dx, ix]), np.stack([by, gy, dy, by]), ("benign", "growth", "decay", "one_inf")


# Form A (k_series_div_a, one lane per series) exists only where a wave's rows fit its LDS budget — gft_series.hip's form_a_waves:
# 2 * (n | 1) <= 160 for f64, n <= 79 — and a request for it at a longer n is answered with form B.  So form A runs at n = 64 (the
# growth and decay exponents of the (64,) row: out of the window at 15, inf at 52; zeros from 54 on), form B there and at the
# issue's three lengths: k_div_1d_wave_batch<4>, <16> and k_div_1d_batch.  Every case asserts the form that ran.
@pytest.mark.parametrize("n,form", [(64, "A"), (64, "B"), (200, "B"), (600, "B"), (1100, "B")])
def test_series_div_items_across_the_switches_bit_exact(n, form, OTP):
    """k_series_div_a / k_div_1d_wave_batch / k_div_1d_batch: every item against the oracle on its own, so that a redo in one
    item cannot disturb its neighbour unnoticed"""
    torch = pytest.importorskip("torch")
    import genfer_amd
    from genfer_amd import series

    genfer_amd.init(0)
    x, y, names = series_batch(n)
    series.set_form(form)
    try:
        got = series.div(torch.from_numpy(x).to("cuda"), torch.from_numpy(y).to("cuda"), n=n).cpu().numpy()
        ran = series.last_form()
    finally:
        series.set_form(None)
    assert ran == form, f"series.div n = {n}: asked for form {form}, form {ran} ran"
    for b, name in enumerate(names):
        a, _, _ = rc.oracle_div(OTP, ("series", n, name), x[b], y[b], [n])
        want = np.zeros(n)
        want[:a.size] = a
        msg = rc.describe_mismatch(f"series.div n = {n} form {ran} (asked {form}) item {b} ({name})", want, got[b])
        assert msg is None, msg
