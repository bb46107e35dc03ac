"""Batched trivariate series on device tensors (genfer_amd.series3, gft_series3_mul / div / exp / log) on the MI355X.

Every coefficient of every item carries the oracle's bits wherever the oracle is normative (everywhere but under a divisor of one
stored coefficient), and the model's (tests/_series3_model.py, the definition) elsewhere; a NaN matches a NaN.  The stored result
shape S and its squeezes, views, broadcasting, in-place results, special values, shortcut rows, refusals and the stream contract."""
import ctypes as C

import numpy as np
import pytest

from _series3_oracle import OPS, assert_bits, dense, host_seeds, model_batch, oracle_is_normative, want
from conftest import REL_TOL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64)


def run(op, x, y, n, seed="host", **kw):
    """x: numpy [B, nx0, nx1, nx2] (or a tensor); the batched call"""
    from genfer_amd import series, series3

    tx = x if isinstance(x, torch.Tensor) else dev(x)
    if op in ("mul", "div"):
        got = getattr(series3, op)(tx, y if isinstance(y, torch.Tensor) else dev(y), n=n, **kw)
    else:
        sd = None
        if seed == "host":
            sd = dev(host_seeds(op, x.cpu().numpy() if isinstance(x, torch.Tensor) else x))
        got = getattr(series3, op)(tx, n=n, seed=sd, **kw)
    assert series.last_form() == "B"  # gft_series_last_form() == 2 after a series3 call
    return got


def seeds_of(op, x):
    return host_seeds(op, x) if op in ("exp", "log") else None


def expected(oracle_lib, OTP, op, x, y, n):
    """the oracle's bits where it is normative, else the model's (small items only: the model is plain Python)"""
    if oracle_is_normative(op, x, y):
        return want(oracle_lib, OTP, op, x, y, n), "oracle"
    assert int(np.prod(n)) <= 64
    return model_batch(op, x, y, n, seeds_of(op, x)), "model"


# ---- bit-exact against the oracle ------------------------------------------------------------------------------------------------

# the smallest item with no unit axis; asymmetric; the one-wave boundary of mul (64 and 72 output pairs); the limit; rows on both
# sides of s2_div1d's wave / block switch (512); long leading axes, whose terms take several scratch chunks
SHAPES = [(2, 2, 2), (3, 4, 5), (5, 3, 2), (4, 4, 8), (4, 4, 9), (16, 16, 16), (2, 2, 512), (2, 2, 513), (2, 2, 1024), (64, 8, 8), (8, 64, 8)]
BATCHES = [1, 3, 65, 300]
CPU_BUDGET = 7.0e7  # B * (n0 * n1 * n2)^2 per case: the oracle side stays within seconds


def cases():
    for n in SHAPES:
        N = n[0] * n[1] * n[2]
        for B in BATCHES:
            if N == 4096 and B != 3 or B > 3 and B * float(N) ** 2 > CPU_BUDGET:
                continue
            yield n, B


def compact_shapes(n):
    return (max(1, n[0] // 2), n[1] - 1, n[2]), (n[0] - 1, n[1], max(2, n[2] // 2))


@pytest.mark.parametrize("op", OPS)
def test_bit_exact_against_the_oracle(op, OTP, oracle_lib):
    checked = 0
    for n, B in cases():
        for xs, ys in [(n, n)] + ([compact_shapes(n)] if B == 3 else []):
            x = dense((B,) + xs, 1000 * n[0] + 10 * n[1] + n[2] + B)
            y = dense((B,) + ys, 2000 * n[0] + 10 * n[1] + n[2] + B + 7)
            assert oracle_is_normative(op, x, y)
            got = run(op, x, y, n)
            assert_bits(got, want(oracle_lib, OTP, op, x, y, n), f"{op} n={n} B={B} x{xs} y{ys}")
            checked += 1
    assert checked >= 35


# stored unit axes under longer result axes, so that S != n; every squeeze of S (one, two and three unit axes)
S_CASES = [((4, 2, 1), (5, 3, 2), (5, 3, 2)), ((4, 2, 2), (4, 1, 2), (4, 3, 2)), ((2, 2, 1), (2, 1, 1), (4, 3, 2)), ((1, 3, 2), (2, 1, 2), (3, 3, 3)),
           ((3, 3, 3), (1, 1, 1), (3, 3, 3)), ((2, 3, 1), (1, 1, 1), (3, 3, 2))]
SQUEEZES = [(3, 1, 4), (3, 4, 1), (1, 3, 4), (4, 1, 1), (1, 1, 5), (1, 1, 1)]


@pytest.mark.parametrize("op", OPS)
def test_stored_result_shape_and_squeezes(op, OTP, oracle_lib):
    from _series3_model import result_shape

    by = {"oracle": 0, "model": 0}
    differs = 0
    for xs, ys, n in S_CASES + [(n, n, n) for n in SQUEEZES]:
        x, y = dense((3,) + xs, 100 * n[0] + sum(xs)), dense((3,) + ys, 200 * n[1] + sum(ys))
        exp, who = expected(oracle_lib, OTP, op, x, y, n)
        got = run(op, x, y, n)
        assert_bits(got, exp, f"{op} x{xs} y{ys} n={n} against the {who}")
        by[who] += 1
        s = result_shape(op, n, xs, ys)
        differs += s != n
        outside = got.cpu().numpy().copy()
        outside[:, :s[0], :s[1], :s[2]] = 0.0
        assert not outside.any() and not np.signbit(outside).any(), (op, n, "outside S is +0.0")
    assert differs >= 1 and by["oracle"] >= 8 and (by["model"] > 0) == (op == "div")


# ---- device seeds ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,B", [((3, 4, 5), 65), ((1, 3, 4), 3), ((4, 4, 9), 3)])
def test_device_seeds(n, B, OTP, oracle_lib):
    """only what depends on coefficient 0 may differ: exp within a few ulps everywhere, log at [0, 0, 0] alone"""
    x = dense((B,) + n, 31 * n[0] + B)
    for op in ("exp", "log"):
        exp = want(oracle_lib, OTP, op, x, None, n)
        got = run(op, x, None, n, seed=None).cpu().numpy()
        if op == "log":
            g, w = got.copy(), exp.copy()
            g[:, 0, 0, 0] = w[:, 0, 0, 0] = 0.0
            assert_bits(g, w, f"log n={n} B={B} device seed, all but [0, 0, 0]")
            got, exp = got[:, :1, :1, :1], exp[:, :1, :1, :1]
        assert np.all(np.abs(got - exp) <= REL_TOL * np.abs(exp)), (op, n, B, np.max(np.abs(got - exp) / np.abs(exp)))


# ---- views -----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,batch", [((3, 4, 5), (4, 5)), ((4, 4, 9), (2, 3))])
def test_views(n, batch, OTP, oracle_lib):
    from genfer_amd import series3

    B, nb = int(np.prod(batch)), len(batch)
    x, y = dense((B,) + n, 11), dense((B,) + n, 12)
    exp = {op: want(oracle_lib, OTP, op, x, y, n).reshape(batch + n) for op in OPS}
    X, Y = dev(x).reshape(batch + n), dev(y).reshape(batch + n)
    seeds = {op: dev(host_seeds(op, x)).reshape(batch) for op in ("exp", "log")}

    def call(op, a, b, **kw):
        return getattr(series3, op)(a, b, **kw) if op in ("mul", "div") else getattr(series3, op)(a, seed=seeds[op], **kw)

    # non-contiguous slab and row strides: a slice of a wider tensor on all three series axes
    wide = torch.zeros(batch + (n[0] + 2, n[1] + 3, n[2] + 9), dtype=torch.float64, device=DEV)
    wide[..., 1:1 + n[0], 2:2 + n[1], 4:4 + n[2]] = X
    xs = wide[..., 1:1 + n[0], 2:2 + n[1], 4:4 + n[2]]
    assert not xs.is_contiguous() and xs.stride(-2) == n[2] + 9 and xs.stride(-3) == (n[1] + 3) * (n[2] + 9)
    for op in OPS:
        assert_bits(call(op, xs, Y), exp[op], f"{op} sliced x")
    # a transposed batch
    perm = tuple(reversed(range(nb))) + (nb, nb + 1, nb + 2)
    xp = X.permute(*perm).contiguous().permute(*perm)
    assert not xp.is_contiguous() and xp.stride(-1) == 1
    for op in OPS:
        assert_bits(call(op, xp, Y), exp[op], f"{op} permuted x")
    # an out= view with guard words around it, intact afterwards
    for op in OPS:
        big = torch.full(batch + (n[0] + 2, n[1] + 2, n[2] + 5), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
        out = big[..., 1:1 + n[0], 1:1 + n[1], 2:2 + n[2]]
        assert call(op, xs, Y, out=out) is out
        assert_bits(out, exp[op], f"{op} sliced out")
        g = big.view(torch.int64).clone()
        g[..., 1:1 + n[0], 1:1 + n[1], 2:2 + n[2]] = GUARD
        assert bool((g == GUARD).all()), op
    # batch stride 0: one item against the batch, on either side; a slab and a row repeated inside an item
    y0 = np.repeat(y[:1], B, axis=0)
    ye = dev(y[:1]).reshape((1,) * nb + n).expand(batch + n)
    assert ye.stride(0) == 0
    assert_bits(series3.mul(X, ye), want(oracle_lib, OTP, "mul", x, y0, n).reshape(batch + n), "mul expanded y")
    assert_bits(series3.div(X, dev(y[0])), want(oracle_lib, OTP, "div", x, y0, n).reshape(batch + n), "div broadcast y")
    assert_bits(series3.div(ye, X), want(oracle_lib, OTP, "div", y0, x, n).reshape(batch + n), "div expanded x")
    xrep = np.broadcast_to(x[:, :1, :1], x.shape).copy()
    xr = dev(x[:, :1, :1]).reshape(batch + (1, 1, n[2])).expand(batch + n)
    assert xr.stride(-2) == 0 and xr.stride(-3) == 0
    assert_bits(series3.mul(xr, Y), want(oracle_lib, OTP, "mul", xrep, y, n).reshape(batch + n), "mul with slab and row strides of 0")
    # in place
    for op in OPS:
        xi = X.clone()
        assert call(op, xi, Y, out=xi) is xi
        assert_bits(xi, exp[op], f"{op} in place on x")
    for op in ("mul", "div"):
        yi = Y.clone()
        call(op, X, yi, out=yi)
        assert_bits(yi, exp[op], f"{op} in place on y")
        wi = wide.clone()  # in place on a strided view
        v = wi[..., 1:1 + n[0], 2:2 + n[1], 4:4 + n[2]]
        call(op, v, Y, out=v)
        assert_bits(v, exp[op], f"{op} in place on a sliced x")
    # a result whose S is smaller than n through a strided out: the zero fill goes through the strides too
    xc = dense((B, 2, 2, 1), 13)
    big = torch.full(batch + (n[0] + 2, n[1] + 2, n[2] + 5), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
    out = big[..., 1:1 + n[0], 1:1 + n[1], 2:2 + n[2]]
    series3.mul(dev(xc).reshape(batch + (2, 2, 1)), dev(xc).reshape(batch + (2, 2, 1)), n=n, out=out)
    assert_bits(out, want(oracle_lib, OTP, "mul", xc, xc, n).reshape(batch + n), "mul S < n into a sliced out")
    g = big.view(torch.int64).clone()
    g[..., 1:1 + n[0], 1:1 + n[1], 2:2 + n[2]] = GUARD
    assert bool((g == GUARD).all())


def test_default_orders_and_empty_batch(oracle_lib, OTP):
    from genfer_amd import series3

    x, y = dense((5, 3, 2, 6), 61), dense((5, 2, 4, 2), 62)
    assert_bits(series3.mul(dev(x), dev(y)), want(oracle_lib, OTP, "mul", x, y, (3, 4, 6)), "mul default n")
    assert_bits(series3.div(dev(x), dev(y), n=(4, 5, 7)), want(oracle_lib, OTP, "div", x, y, (4, 5, 7)), "div n beyond both")
    assert_bits(run("exp", x, None, (4, 3, 7)), want(oracle_lib, OTP, "exp", x, None, (4, 3, 7)), "exp n beyond x")
    assert_bits(run("log", x, None, (4, 3, 7)), want(oracle_lib, OTP, "log", x, None, (4, 3, 7)), "log n beyond x")
    e = torch.zeros((0, 3, 2, 8), dtype=torch.float64, device=DEV)
    assert series3.mul(e, e).shape == (0, 3, 2, 8) and series3.exp(e).shape == (0, 3, 2, 8) and series3.div(e, e).shape == (0, 3, 2, 8)


# ---- special values and shortcut rows ----------------------------------------------------------------------------------------------

INF, NAN = float("inf"), float("nan")


def test_special_values():
    """infinities, NaNs, exact zeros and negative zeros follow the definition bit for bit (a NaN for a NaN); only stored
    coefficients enter a sum, so a compact operand next to an infinity leaves the coefficients it does not reach finite"""
    from genfer_amd import series3

    n = (3, 3, 4)
    plain = dense(n, 71)
    items = []
    for (i, j, k, v) in [(1, 1, 1, INF), (0, 0, 2, -INF), (2, 0, 0, NAN), (0, 2, 3, INF)]:
        a = plain.copy()
        a[i, j, k] = v
        items.append(a)
    z = plain.copy()
    z[1:] = 0.0
    z[0, 1:] = -0.0
    items += [z, -z, plain]
    x = np.stack(items)
    x[:, 0, 0, 0] = np.abs(plain[0, 0, 0])  # seeds the host libm can form
    y = np.stack(items[::-1])
    y[:, 0, 0, 0] = 1.25
    with np.errstate(all="ignore"):
        for op in OPS:
            got = run(op, x, y, n)
            assert_bits(got, model_batch(op, x, y, n, seeds_of(op, x)), f"{op} specials")
            alone = run(op, x[-1:], y[-1:], n)
            assert torch.equal(bits(alone), bits(got[-1:])), (op, "the plain item inside the batch of specials")
        y0 = y.copy()
        y0[:, 0, 0, 0] = [0.0, -0.0, INF, NAN, 0.0, -0.0, 1.0]
        assert_bits(run("div", x, y0, n), model_batch("div", x, y0, n), "div by y[0, 0, 0] in {0, -0, inf, nan}")
        # compact x of (2, 2, 2) with an infinity in its corner: it reaches the outputs with every index >= 1 only
        xc = dense((3, 2, 2, 2), 72)
        xc[:, 1, 1, 1] = INF
        yd = dense((3,) + n, 73)
        for op in ("mul", "div"):
            got = getattr(series3, op)(dev(xc), dev(yd), n=n).cpu().numpy()
            assert_bits(got, model_batch(op, xc, yd, n), f"{op} compact x with an infinity")
            assert np.isfinite(got[:, 0]).all() and np.isfinite(got[:, :, 0]).all() and np.isfinite(got[:, :, :, 0]).all()
            assert not np.isfinite(got[:, 1:, 1:, 1:]).any()


def test_shortcut_rows_take_the_general_loops():
    """zero, one, constant and linear operands and a constant divisor -- what the operator wrappers shortcut -- give the general
    loops, and every item alone equals the item inside the batch"""
    n = (3, 3, 3)
    plain = dense(n, 81)
    zero, one, const, lin = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    one[0, 0, 0] = 1.0
    const[0, 0, 0] = 2.5
    lin[0, 0, 0], lin[0, 0, 1], lin[1, 0, 0] = 1.5, 0.75, -0.5
    x = np.stack([zero, one, const, lin, plain, plain])
    y = np.stack([plain, plain, plain, plain, const, lin])  # (divisors with y[0, 0, 0] != 0)
    xpos = x.copy()
    xpos[0, 0, 0, 0] = 1.0  # log of the zero item: keep a positive coefficient 0
    with np.errstate(all="ignore"):
        for op in OPS:
            a = xpos if op == "log" else x
            got = run(op, a, y, n)
            assert_bits(got, model_batch(op, a, y, n, seeds_of(op, a)), f"{op} shortcut rows")
            for b in range(a.shape[0]):
                assert torch.equal(bits(run(op, a[b:b + 1], y[b:b + 1], n)), bits(got[b:b + 1])), (op, b)


# ---- refusals through the C entry points -----------------------------------------------------------------------------------------


def test_c_entry_point_refusals():
    from genfer_amd import series3
    import genfer_amd

    x = torch.rand((6, 2, 4, 16), dtype=torch.float64, device=DEV) + 0.5
    y = torch.rand((6, 2, 4, 16), dtype=torch.float64, device=DEV) + 0.5

    def after():  # no stale HIP error: torch's next call succeeds
        assert float((x + 1.0).sum().item()) > 0

    series3.mul(x, y)  # declares the entry points
    L = genfer_amd.lib()
    one = (C.c_size_t * 1)(6)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    big = torch.zeros(6 * 4097, dtype=torch.float64, device=DEV)

    def c_mul(nx, ny, nr, rss=None, rrs=None, xss=64, res=big):
        return L.gft_series3_mul(vp(x), None, xss, 16, *nx, vp(y), None, 64, 16, *ny, vp(res), None, nr[1] * nr[2] if rss is None else rss,
                                 nr[2] if rrs is None else rrs, *nr, one, 1, None)

    full = (2, 4, 16)
    for args, kw, text in [((full, full, (17, 241, 1)), {}, "n0 * n1 * n2 = 17 * 241 * 1 exceeds the limit of 4096"),
                           ((full, full, (2, 0, 16)), {}, "n0 * n1 * n2 == 0"),
                           ((full, full, (2, 3, 16)), {}, "x has 2 x 4 x 16 coefficients, the result 2 x 3 x 16"),
                           (((2, 4, 0), full, full), {}, "an operand has no coefficients"),
                           ((full, full, full), {"rrs": -16}, "negative strides"),
                           ((full, full, full), {"rss": -64}, "negative strides"),
                           ((full, full, full), {"xss": -64}, "negative strides"),
                           ((full, full, full), {"rss": 0}, "zero slab stride"),
                           ((full, full, full), {"rrs": 0}, "zero row stride"),
                           ((full, full, full), {"rss": 32}, "overlap each other"),
                           ((full, full, full), {"res": x[0, 0, 1]}, "partially overlaps x")]:
        assert c_mul(*args, **kw) == -1 and text in L.gft_last_error().decode(), (text, L.gft_last_error())
        after()
    assert L.gft_series3_exp(vp(x), None, 64, 16, 2, 4, 16, None, None, None, None, 64, 16, 2, 4, 16, one, 1, None) == -1
    assert "series3_exp: the result is a null pointer" in L.gft_last_error().decode()
    after()
    assert c_mul(full, full, full) == 0
    after()
    # the limit itself runs in every orientation, and the calls after the refusals are unharmed
    for n in [(16, 16, 16), (1, 1, 4096), (4096, 1, 1), (1, 4096, 1), (2, 1, 2048), (2, 2048, 1)]:
        a = torch.rand((2,) + n, dtype=torch.float64, device=DEV) + 0.5
        for op in OPS:
            assert getattr(series3, op)(a, a).shape == (2,) + n if op in ("mul", "div") else getattr(series3, op)(a).shape == (2,) + n
    assert torch.equal(bits(series3.mul(x, y)), bits(series3.mul(x.clone(), y.clone())))


# ---- streams ---------------------------------------------------------------------------------------------------------------------


def test_side_stream_is_ordered_with_torchs_work(oracle_lib, OTP):
    from genfer_amd import series3

    B, n = 512, (2, 3, 4)
    x, y = dense((B,) + n, 41), dense((B,) + n, 42)
    exp = want(oracle_lib, OTP, "mul", x, y, n)
    X, Y = dev(x), dev(y)
    src = torch.zeros((B,) + n, dtype=torch.float64, device=DEV)
    series3.mul(src, Y)  # warm the kernel
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(20_000_000)  # the operand is produced behind a long kernel on this stream
        src.copy_(X)
        z = series3.mul(src, Y)
        twice = z * 2.0  # consumed right after, no host synchronisation in between
        src.zero_()  # the operand is reused right after
    s.synchronize()
    assert_bits(z, exp, "mul on a side stream")
    assert_bits(twice, exp * 2.0, "consumer on the side stream")
