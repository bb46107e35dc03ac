"""Batched bivariate interval series on device tensors (genfer_amd.interval_series2, gfti_series2_*) on the MI355X.

Every bound of every coefficient of every item is compared bit for bit (a NaN for a NaN) with the oracle's Interval<F64>: the raw
product of tests/series2_interval_oracle.cpp for mul, the handle operators for div / exp / log where they are normative and the
model of tests/_series2_interval_model.py elsewhere, 3.17's chains over that product for compose and pow (all pinned to each other on
the CPU by tests/test_interval_series2_cpu.py).  Views, in-place results, refusals, the limit and the stream contract; and a guard
that the f64 family, whose kernels are now instantiations of the same bodies, still gives the f64 oracle's bits."""
import numpy as np
import pytest

import _series2_compose_cases as cc
import _series2_oracle as f64o
from _series2_oracle import compact_shapes
from conftest import REL_TOL
from test_interval_series2_cpu import (assert_bits, data2, host_seeds, is_normative, shim2, want_compose, want_handle,  # noqa: F401
                                       want_model, want_mul, want_pow)
from test_interval_series_cpu import _device_like

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 0x5A5A5A5A5A5A5A5A
OPS = ("mul", "div", "exp", "log")
KINDS = ("pos", "mixed", "special")
# smallest items; odd N (the middle output of the pairing); 288 output pairs on 256 lanes (the stride loop); pass-1 scratch smaller
# than the late rows' terms at (64, 32); s2_div1d's block form (n1 > 512); off wave multiples; the limit both ways
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (3, 5), (8, 8), (16, 16), (24, 24), (5, 64), (64, 5), (9, 65), (65, 9), (32, 64), (64, 32),
          (3, 640), (2, 1024), (1024, 2)]
MODEL_MAX = 20  # coefficients per item the scalar model is used on (every step is a ctypes call)
CPU_BUDGET = 7.0e7  # B * slices * (n0 * n1)^2 per compose case, tests/test_series2_compose_gpu.py's budget


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64)


def ivs2():
    from genfer_amd import interval_series2

    return interval_series2


LDS_REFUSALS = []


def run(op, X, Y, n, seeds=None, **kw):
    """X: numpy [2, B, nx0, nx1] or a tensor; Y likewise (mul, div).  Where the runtime grants only 64 KB of LDS an item that needs
    more is refused by name; that refusal is returned as None (and recorded), anything else raises"""
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    tx = X if isinstance(X, torch.Tensor) else dev(X)
    try:
        if op in ("mul", "div"):
            got = getattr(ivs2(), op)(tx, Y if isinstance(Y, torch.Tensor) else dev(Y), n=n, **kw)
        else:
            got = getattr(ivs2(), op)(tx, n=n, seed=None if seeds is None else dev(seeds), **kw)
    except TaylorError as e:
        if "bytes of LDS" in str(e) and "the runtime grants 65536 bytes" in str(e):
            LDS_REFUSALS.append((op, n))
            return None
        raise
    assert series.last_form() == "B"
    return got


def expected(op, X, Y, n, OTPI, oracle_lib, shim):
    """(the expected value, who supplied it, the host seeds)"""
    seeds = host_seeds(oracle_lib, op, X) if op in ("exp", "log") else None
    if op == "mul":
        return want_mul(shim, X, Y, n), "oracle", None
    if is_normative(op, X, Y) and not (op == "exp" and min(X.shape[-2:]) < 2 and not np.isfinite(X).all()):
        return want_handle(OTPI, op, X, Y, n), "oracle", seeds
    assert n[0] * n[1] <= MODEL_MAX
    return want_model(oracle_lib, op, X, Y, n, seeds), "model", seeds


# ---- bit-exact against the oracle ------------------------------------------------------------------------------------------------


def operand_shapes(op, n, kind):
    """dense, and the compact operands (n0 // 2, n1 - 1) / (n0 - 1, max(2, n1 // 2)).  Where the compact divisor / operand of log keeps a
    single coefficient on an axis the oracle is not normative: items of at most MODEL_MAX coefficients are checked against the model,
    larger ones keep that operand dense.  The same for exp of an operand with a single row or column that holds an infinity or a NaN:
    the oracle stores one row or column of the result and leaves the rest +0, the definition multiplies the NaN by the [0,0] there"""
    out = [(n, n)]
    if n != (1, 1):
        xs, ys = compact_shapes(*n)
        small = n[0] * n[1] <= MODEL_MAX
        if op == "div" and min(ys) < 2 and not small:
            ys = n
        if (op == "log" or (op == "exp" and kind == "special")) and min(xs) < 2 and not small:
            xs = n
        if (xs, ys) != (n, n):
            out.append((xs, ys))
    return out


@pytest.mark.parametrize("op", OPS)
def test_bit_exact_against_the_oracle(op, OTPI, oracle_lib, shim2):
    checked = {"oracle": 0, "model": 0}
    for i, n in enumerate(SHAPES):
        N = n[0] * n[1]
        # small items: every kind on 5 items (the five special seeds); large ones: 3 items of one kind, the kinds taking turns
        for kind in (KINDS if N <= 64 else (KINDS[i % 3],)):
            for xs, ys in operand_shapes(op, n, kind):
                B = 5 if N <= 64 else 3
                X, Y = data2(kind, B, xs, 1000 * n[0] + n[1] + B), data2(kind, B, ys, 2000 * n[0] + n[1] + B + 7)
                expect, by, seeds = expected(op, X, Y, n, OTPI, oracle_lib, shim2)
                got = run(op, X, Y, n, seeds)
                if got is None:  # refused by name under a 64 KB grant: only an item whose arrays and one scratch row exceed it
                    assert op != "mul" and N * 32 + n[1] * 16 > 65536, (op, n)
                    continue
                assert_bits(got, expect, f"{op} n={n} B={B} x{xs} y{ys} {kind} against the {by}")
                checked[by] += 1
    assert checked["oracle"] >= 30 and (checked["model"] > 0) == (op != "mul")


@pytest.mark.parametrize("op", ["mul", "div", "exp"])
def test_batches(op, OTPI, oracle_lib, shim2):
    """more items than a wave of workgroups: 65 and 300 items at (8, 8), 65 at (16, 16)"""
    for n, B, kind in [((8, 8), 300, "special"), ((8, 8), 65, "mixed"), ((16, 16), 65, "pos")]:
        X, Y = data2(kind, B, n, 31 * n[0] + B), data2(kind, B, n, 37 * n[0] + B)
        expect, _, seeds = expected(op, X, Y, n, OTPI, oracle_lib, shim2)
        assert_bits(run(op, X, Y, n, seeds), expect, f"{op} n={n} B={B} {kind}")


@pytest.mark.parametrize("op", ["div", "log"])
def test_model_cases(op, oracle_lib):
    """divisors / operands of log with a length-1 axis, where the reference shortcuts or stores fewer rows, and special values: the
    loops of include/gftaylor.h over the oracle's scalar interval operations are the definition"""
    for n in [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (3, 5)]:
        for ts in sorted({(1, n[1]), (n[0], 1), (1, 1), n}):
            for kind in ("mixed", "special"):
                B = 5
                if op == "div":
                    X, Y = data2(kind, B, n, 31 * n[0] + n[1]), data2(kind, B, ts, 37 * n[0] + n[1])
                else:
                    X, Y = data2(kind, B, ts, 41 * n[0] + n[1]), None
                seeds = host_seeds(oracle_lib, op, X) if op == "log" else None
                assert_bits(run(op, X, Y, n, seeds), want_model(oracle_lib, op, X, Y, n, seeds), f"{op} n={n} operand {ts} {kind}")


def test_explicit_orders(OTPI, oracle_lib, shim2):
    """n defaults to the larger stored length on each axis, and may be larger than both operands"""
    X, Y = data2("mixed", 5, (3, 6), 61), data2("mixed", 5, (4, 2), 62)
    assert_bits(ivs2().mul(dev(X), dev(Y)), want_mul(shim2, X, Y, (4, 6)), "mul default n")
    assert_bits(ivs2().mul(dev(X), dev(Y), n=(9, 11)), want_mul(shim2, X, Y, (9, 11)), "mul n beyond both")
    assert_bits(ivs2().div(dev(X), dev(Y), n=(7, 9)), want_handle(OTPI, "div", X, Y, (7, 9)), "div n beyond both")
    for op in ("exp", "log"):
        assert_bits(run(op, X, None, (6, 9), host_seeds(oracle_lib, op, X)), want_handle(OTPI, op, X, None, (6, 9)), f"{op} n beyond x")


# ---- device seeds ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,B", [((8, 8), 65), ((5, 64), 3), ((16, 16), 5)])
def test_device_seeds(n, B, OTPI, oracle_lib):
    X = data2("pos", B, n, 31 * n[0] + B)
    for op in ("exp", "log"):
        expect = want_handle(OTPI, op, X, None, n)
        hosted = run(op, X, None, n, host_seeds(oracle_lib, op, X))
        assert_bits(hosted, expect, f"{op} n={n} B={B} host seeds")
        got = run(op, X, None, n, None).cpu().numpy()
        if op == "log":  # only coefficient [0, 0] depends on the seed
            g, w = got.copy(), expect.copy()
            g[:, :, 0, 0] = w[:, :, 0, 0] = 0.0
            assert_bits(g, w, f"log n={n} B={B} device seed, all but [0, 0]")
            got, expect = got[:, :, :1, :1], expect[:, :, :1, :1]
        assert np.all(np.abs(got - expect) <= REL_TOL * np.abs(expect)), (op, n, B, np.max(np.abs(got - expect) / np.abs(expect)))


# ---- compose and pow ---------------------------------------------------------------------------------------------------------------


def f_shape(n, var, B):
    """f dense while the chain stays within the CPU budget, else three slices"""
    if B * n[var] * float(n[0] * n[1]) ** 2 <= CPU_BUDGET:
        return n
    return (3, n[1]) if var == 0 else (n[0], 3)


@pytest.mark.parametrize("var", [0, 1])
def test_compose_bit_exact(var, oracle_lib, shim2):
    checked = 0
    for i, n in enumerate(SHAPES):
        B = 3
        fs = f_shape(n, var, B)
        cases = [(fs, n, KINDS[i % 3])]
        if n != (1, 1) and n[0] * n[1] <= 1024:
            fc, gc = compact_shapes(*n)
            cases.append(((min(fc[0], fs[0]), min(fc[1], fs[1])), gc, KINDS[(i + 1) % 3]))
        for fsh, gsh, kind in cases:
            F, G = data2(kind, B, fsh, 1000 * n[0] + n[1] + var), data2(kind, B, gsh, 2000 * n[0] + n[1] + 7)
            got = ivs2().compose(dev(F), dev(G), var, n=n)
            assert_bits(got, want_compose(shim2, oracle_lib, F, G, var, n), f"compose var={var} n={n} f{fsh} g{gsh} {kind}")
            checked += 1
    assert checked >= 30


def glds_pair():
    """the smallest (n0, 64) on either side of compose's GLDS decision, by construction: two result arrays and g of 16-byte elements.
    2 N + ng <= 4096 elements fit the 64 KB the runtime always grants (g resident whatever was granted); 2 N + ng > 5120 exceed the
    80 KB request (g in global memory whatever was granted)."""
    resident = max(n0 for n0 in range(1, 33) if 3 * n0 * 64 <= 4096)
    glob = min(n0 for n0 in range(1, 33) if 3 * n0 * 64 > 5120)
    return (resident, 64), (glob, 64)


@pytest.mark.parametrize("var", [0, 1])
def test_compose_both_instantiations_and_corners(var, oracle_lib, shim2):
    B = 3
    for n in glds_pair():
        fs = (3, n[1]) if var == 0 else (n[0], 3)
        F, G = data2("mixed", B, fs, 83 + var), data2("mixed", B, n, 84)
        assert_bits(ivs2().compose(dev(F), dev(G), var, n=n), want_compose(shim2, oracle_lib, F, G, var, n), f"compose var={var} n={n} f{fs} dense g")
    # g in global memory through a row stride of its own
    n = glds_pair()[1]
    wide = torch.zeros((2, B, n[0], n[1] + 16), dtype=torch.float64, device=DEV)
    wide[..., 3:3 + n[1]] = dev(G)
    gv = wide[..., 3:3 + n[1]]
    assert gv.stride(-2) == n[1] + 16
    assert_bits(ivs2().compose(dev(F), gv, var, n=n), want_compose(shim2, oracle_lib, F, G, var, n), f"compose var={var} n={n}, strided g in global memory")
    # one-slice f; g of stored shape (2, 2), (1, 1), a single row, a single column
    for n in [(3, 5), (8, 8), (16, 16)]:
        k = n[1 - var]
        one = (1, k) if var == 0 else (k, 1)
        for fs, gs in [(one, n), (n, (2, 2)), (n, (1, 1)), (n, (1, n[1])), (n, (n[0], 1))]:
            F, G = data2("special", 5, fs, 300 * n[0] + fs[0] + var), data2("special", 5, gs, 500 * n[1] + gs[1] + var)
            assert_bits(ivs2().compose(dev(F), dev(G), var, n=n), want_compose(shim2, oracle_lib, F, G, var, n), f"compose var={var} n={n} f{fs} g{gs}")


POW_E = [0, 1, 2, 3, 5]


@pytest.mark.parametrize("n,B,kind", [((1, 1), 5, "mixed"), ((2, 2), 5, "special"), ((3, 5), 5, "special"), ((8, 8), 300, "special"), ((24, 24), 3, "mixed"),
                                      ((9, 65), 3, "pos"), ((64, 32), 3, "mixed")])
def test_pow_bit_exact(n, B, kind, shim2):
    X = data2(kind, B, n, 900 * n[0] + n[1])
    xc = compact_shapes(*n)[0]
    Xc = data2(kind, B, xc, 901 * n[0] + n[1])
    for e in POW_E:
        assert_bits(ivs2().pow(dev(X), e), want_pow(shim2, X, e, n), f"pow n={n} B={B} e={e} {kind}")
        if e in (2, 5) and B <= 5:
            assert_bits(ivs2().pow(dev(Xc), e, n=n), want_pow(shim2, Xc, e, n), f"pow n={n} compact x{xc} e={e}")


# ---- views -----------------------------------------------------------------------------------------------------------------------


def call(op, a, b, seeds, **kw):
    m = ivs2()
    if op in ("mul", "div"):
        return getattr(m, op)(a, b, **kw)
    if op == "compose":
        return m.compose(a, b, 1, **kw)
    if op == "pow":
        return m.pow(a, 3, **kw)
    return getattr(m, op)(a, seed=seeds[op], **kw)


ALL = OPS + ("compose", "pow")


@pytest.mark.parametrize("n,batch", [((3, 5), (4, 5)), ((16, 16), (7,))])
def test_views(n, batch, OTPI, oracle_lib, shim2):
    B, nb = int(np.prod(batch)), len(batch)
    X, Y = data2("mixed", B, n, 11), data2("mixed", B, n, 12)
    full = (2,) + batch + n

    def expect_all(X, Y):
        e = {op: expected(op, X, Y, n, OTPI, oracle_lib, shim2)[0] for op in OPS}
        e["compose"] = want_compose(shim2, oracle_lib, X, Y, 1, n)
        e["pow"] = want_pow(shim2, X, 3, n)
        return {k: v.reshape(full) for k, v in e.items()}

    expect = expect_all(X, Y)
    tX, tY = dev(X).reshape(full), dev(Y).reshape(full)
    seeds = {op: dev(host_seeds(oracle_lib, op, X)).reshape((2,) + batch) for op in ("exp", "log")}
    # a row stride > n1: a slice of a wider tensor on both series axes
    wide = torch.zeros((2,) + batch + (n[0] + 3, n[1] + 9), dtype=torch.float64, device=DEV)
    wide[..., 1:1 + n[0], 4:4 + n[1]] = tX
    xs = wide[..., 1:1 + n[0], 4:4 + n[1]]
    assert xs.stride(-2) == n[1] + 9
    for op in ALL:
        assert_bits(call(op, xs, tY, seeds), expect[op], f"{op} sliced x")
    # the planes interleaved per item: [B..., 2, n0, n1] in memory
    inter = tX.movedim(0, nb).contiguous().movedim(nb, 0)
    assert inter.stride(0) == n[0] * n[1] and inter.stride(nb) == 2 * n[0] * n[1]
    for op in ALL:
        assert_bits(call(op, inter, tY, seeds), expect[op], f"{op} interleaved planes")
    oi = torch.empty(batch + (2,) + n, dtype=torch.float64, device=DEV).movedim(nb, 0)
    for op in ALL:
        assert call(op, tX, tY, seeds, out=oi) is oi
        assert_bits(oi, expect[op], f"{op} out with interleaved planes")
    # plane stride 0: point intervals, no copy (seeds too)
    P = np.stack([X[0], X[0]])
    pe = dev(X[0]).reshape(batch + n).expand(full)
    assert pe.stride(0) == 0
    ep = expect_all(P, Y)
    ps = {op: dev(host_seeds(oracle_lib, op, P)).reshape((2,) + batch) for op in ("exp", "log")}
    for op in ALL:
        assert_bits(call(op, pe, tY, ps), ep[op], f"{op} x with plane stride 0")
    assert_bits(ivs2().mul(tY, pe), want_mul(shim2, Y, P, n).reshape(full), "mul y with plane stride 0")
    # a stride-0 batch axis: one item against the batch, on either side
    Y0 = np.repeat(Y[:, :1], B, axis=1)
    ye = dev(Y[:, :1]).reshape((2,) + (1,) * nb + n).expand(full)
    assert ye.stride(1) == 0
    assert_bits(ivs2().mul(tX, ye), want_mul(shim2, X, Y0, n).reshape(full), "mul expanded y")
    assert_bits(ivs2().div(tX, dev(Y[:, 0])), want_handle(OTPI, "div", X, Y0, n).reshape(full), "div broadcast y")
    assert_bits(ivs2().div(ye, tX), want_handle(OTPI, "div", Y0, X, n).reshape(full), "div expanded x")
    # an out= view with guard words around it, intact afterwards
    for op in ALL:
        big = torch.full((2,) + batch + (n[0] + 2, n[1] + 5), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
        out = big[..., 1:1 + n[0], 2:2 + n[1]]
        assert call(op, xs, tY, seeds, out=out) is out
        assert_bits(out, expect[op], f"{op} sliced out")
        g = big.view(torch.int64).clone()
        g[..., 1:1 + n[0], 2:2 + n[1]] = GUARD
        assert bool((g == GUARD).all()), op
    # in place: the result as the same view of an operand
    for op in ALL:
        xi = tX.clone()
        assert call(op, xi, tY, seeds, out=xi) is xi
        assert_bits(xi, expect[op], f"{op} in place on x")
        ii = inter.clone()  # (clone keeps the interleaved strides)
        if ii.stride() == inter.stride():
            call(op, ii, tY, seeds, out=ii)
            assert_bits(ii, expect[op], f"{op} in place on interleaved x")
    for op in ("mul", "div", "compose"):
        yi = tY.clone()
        call(op, tX, yi, seeds, out=yi)
        assert_bits(yi, expect[op], f"{op} in place on y")
        wi = wide.clone()
        v = wi[..., 1:1 + n[0], 4:4 + n[1]]
        call(op, v, tY, seeds, out=v)
        assert_bits(v, expect[op], f"{op} in place on a sliced x")


def test_empty_batch_is_a_no_op():
    e = torch.zeros((2, 0, 3, 8), dtype=torch.float64, device=DEV)
    m = ivs2()
    assert m.mul(e, e).shape == (2, 0, 3, 8) and m.exp(e).shape == (2, 0, 3, 8) and m.pow(e, 3).shape == (2, 0, 3, 8)
    assert m.compose(e, e, 1).shape == (2, 0, 3, 8)


# ---- refusals and limits -----------------------------------------------------------------------------------------------------------


def test_refusals_and_limits():
    from genfer_amd.taylor import TaylorError

    m = ivs2()
    x = torch.rand((2, 6, 4, 16), dtype=torch.float64, device=DEV) + 0.5
    y = torch.rand((2, 6, 4, 16), dtype=torch.float64, device=DEV) + 0.5

    def after():  # no stale HIP error: torch's next call succeeds
        assert float((x + 1.0).sum().item()) > 0

    with pytest.raises(TaylorError, match="zero plane stride"):
        m.mul(x, y, out=torch.empty((1, 6, 4, 16), dtype=torch.float64, device=DEV).expand(2, 6, 4, 16))
    after()
    with pytest.raises(TaylorError, match="zero stride"):
        m.mul(x, y, out=torch.empty((2, 1, 4, 16), dtype=torch.float64, device=DEV).expand(2, 6, 4, 16))
    with pytest.raises(TaylorError, match="zero row stride"):
        m.mul(x, y, out=torch.empty((2, 6, 1, 16), dtype=torch.float64, device=DEV).expand(2, 6, 4, 16))
    with pytest.raises(TaylorError, match="overlap"):  # the planes 32 apart, an item 64 long: the planes overlap each other
        m.mul(x, y, out=torch.empty(2048, dtype=torch.float64, device=DEV).as_strided((2, 6, 4, 16), (32, 64, 16, 1)))
    after()
    # a partial overlap with an operand is refused, by address range over both planes
    buf = torch.rand((2, 6, 4, 40), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps x"):
        m.mul(buf[..., 0:16], y, out=buf[..., 8:24])
    with pytest.raises(TaylorError, match="partially overlaps y"):
        m.div(x, buf[..., 0:16], out=buf[..., 16:32])
    with pytest.raises(TaylorError, match="partially overlaps x"):  # the same memory with another plane stride is not the same view
        m.exp(buf[:1].expand(2, 6, 4, 40)[..., :16], out=buf[..., :16])
    sd = torch.rand((2, 6, 4, 16), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps the seeds"):
        m.exp(x, seed=sd[:, :, 0, 0], out=sd)
    after()
    # 2049 coefficients: by Python, and by the library through the C entry point
    with pytest.raises(TaylorError, match="= 2049 exceeds the limit of 2048"):
        m.mul(x, y, n=(3, 683))
    import ctypes as C

    import genfer_amd

    m.mul(x, y)  # declares the entry points
    L = genfer_amd.lib()
    one = (C.c_size_t * 1)(6)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    big = torch.zeros(2 * 6 * 2049, dtype=torch.float64, device=DEV)

    def c_mul(nr):
        return L.gfti_series2_mul(vp(x), None, 16, 4, 16, vp(y), None, 16, 4, 16, vp(big), None, nr[1], nr[0], nr[1], one, 1, None)

    assert c_mul((3, 683)) == -1 and "n0 * n1 = 3 * 683 exceeds the limit of 2048" in L.gft_last_error().decode()
    assert c_mul((0, 16)) == -1 and "n0 * n1 == 0" in L.gft_last_error().decode()
    assert c_mul((4, 16)) == 0
    after()
    # tensors on different devices
    if torch.cuda.device_count() > 1:
        other = torch.zeros((2, 6, 4, 16), dtype=torch.float64, device="cuda:1")
    else:
        class Elsewhere(torch.Tensor):
            @property
            def device(self):
                return torch.device("cuda", 1)

        other = torch.zeros((2, 6, 4, 16), dtype=torch.float64, device="meta").as_subclass(Elsewhere)
    with pytest.raises(TaylorError, match="different devices"):
        m.mul(x, other)
    with pytest.raises(TaylorError, match="different devices"):
        m.mul(x, y, out=other)
    after()
    # the limit itself runs (both ways), and the calls after the refusals are unharmed
    for n in [(32, 64), (1, 2048), (2048, 1)]:
        a = torch.rand((2, 2) + n, dtype=torch.float64, device=DEV) + 0.5
        assert m.mul(a, a).shape == (2, 2) + n
    assert torch.equal(bits(m.mul(x, y)), bits(m.mul(x.clone(), y.clone())))


# ---- streams ---------------------------------------------------------------------------------------------------------------------


def _sleep_cycles_for_ms(ms):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(1_000_000)
    b.record()
    b.synchronize()
    per_ms = 1_000_000 / max(a.elapsed_time(b), 1e-3)
    return int(min(per_ms * ms, 2**40))


def test_stream_ordered_without_host_stall(shim2):
    B, n = 512, (4, 6)
    X, Y = data2("mixed", B, n, 41), data2("mixed", B, n, 42)
    expect = want_mul(shim2, X, Y, n)
    tX, tY = dev(X), dev(Y)
    src = torch.zeros((2, B) + n, dtype=torch.float64, device=DEV)
    ivs2().mul(src, tY)  # warm the kernel
    cycles = _sleep_cycles_for_ms(100)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        src.copy_(tX)  # the operand is produced behind a long kernel on this stream
        z = ivs2().mul(src, tY)
        done = torch.cuda.Event()
        done.record()
        returned_early = not done.query()  # allowed to be false, never required
        twice = z * 2.0  # consumed right after, no host synchronisation in between
        src.zero_()  # the operand is reused right after
    s.synchronize()
    assert_bits(z, expect, "mul on a side stream")
    assert_bits(twice, expect * 2.0, "consumer on a side stream")
    assert returned_early in (True, False)


# ---- the f64 family after the refactor -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [(16, 16), (9, 65)])
def test_f64_family_keeps_the_oracle_bits(n, OTP, oracle_lib):
    from genfer_amd import series2

    B = 3
    x, y = f64o.dense((B,) + n, 1000 * n[0] + n[1] + B), f64o.signed((B,) + n, 2000 * n[0] + n[1] + B + 7)
    for op in f64o.OPS:
        if op in ("mul", "div"):
            got = getattr(series2, op)(dev(x), dev(y))
        else:
            got = getattr(series2, op)(dev(x), seed=dev(f64o.host_seeds(op, x)))
        f64o.assert_bits(got, f64o.want(oracle_lib, OTP, op, x, y, n), f"series2.{op} n={n}")
    fs = (4, n[1])
    f = f64o.dense((B,) + fs, 83)
    for var in (0, 1):
        ff = f if var == 0 else f64o.dense((B, n[0], 4), 85)
        f64o.assert_bits(series2.compose(dev(ff), dev(y), var, n=n), cc.want_compose(oracle_lib, ff, y, var, n), f"series2.compose var={var} n={n}")
    for e in (0, 1, 2, 3, 5):
        f64o.assert_bits(series2.pow(dev(x), e), cc.want_pow(oracle_lib, x, e, n), f"series2.pow n={n} e={e}")
