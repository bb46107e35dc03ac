"""Batched bivariate series on device tensors (genfer_amd.series2, gft_series2_mul / div / exp / log) on the MI355X.

Every coefficient of every item carries the oracle's bits wherever the oracle is normative, and the model's
(tests/_series2_model.py, the definition) elsewhere; views, broadcasting, in-place results, special values, refusals, the limits
and the stream contract."""
import ctypes as C

import numpy as np
import pytest

import _series2_model as model
from _series2_oracle import OPS, assert_bits, compact_shapes, dense, host_seeds, oracle_is_normative, want, want_handle
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
    """x: numpy [B, nx0, nx1] (or a tensor); the batched call"""
    from genfer_amd import series, series2

    tx = x if isinstance(x, torch.Tensor) else dev(x)
    if op in ("mul", "div"):
        got = getattr(series2, op)(tx, y if isinstance(y, torch.Tensor) else dev(y), n=n, **kw)
    else:
        sd = None
        if seed == "host":
            sd = dev(host_seeds(op, x.cpu().numpy() if isinstance(x, torch.Tensor) else x))
        got = getattr(series2, op)(tx, n=n, seed=sd, **kw)
    assert series.last_form() == "B"  # gft_series_last_form() == 2 after a series2 call
    return got


def model_batch(op, x, y, n):
    f = getattr(model, op)
    return np.stack([f(x[b], y[b], n) if op in ("mul", "div") else f(x[b], n) for b in range(x.shape[0])])


# ---- bit-exact against the oracle ------------------------------------------------------------------------------------------------

# a one-wave workgroup, rows longer than a wave, items at the 4096 limit both ways, degenerate axes
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (8, 8), (16, 16), (5, 64), (64, 5), (9, 65), (65, 9), (64, 64), (2, 2048), (2048, 2)]
BATCHES = [1, 3, 65, 300]
CPU_BUDGET = 7.0e7  # B * (n0 * n1)^2 per case: the oracle side stays within seconds (test_series_batch_gpu.py's budget)


def cases():
    for n in SHAPES:
        for B in BATCHES:
            if B > 3 and B * float(n[0] * n[1]) ** 2 > CPU_BUDGET:
                continue
            yield n, B


def operand_shapes(op, n, B):
    """dense, and on the batches of 3 and 65 the compact operands (n0 // 2, n1 - 1) / (n0 - 1, max(2, n1 // 2)).  Where the
    compact divisor / operand of log keeps a single coefficient on an axis the oracle is not normative: items of at most 64
    coefficients are then checked against the model, larger ones keep that operand dense (the model is plain Python)."""
    out = [(n, n)]
    if B in (3, 65) and n != (1, 1):
        xs, ys = compact_shapes(*n)
        small = n[0] * n[1] <= 64
        if op == "div" and min(ys) < 2 and not small:
            ys = n
        if op == "log" and min(xs) < 2 and not small:
            return out
        out.append((xs, ys))
    return out


@pytest.mark.parametrize("op", OPS)
def test_bit_exact_against_the_oracle(op, OTP, oracle_lib):
    checked = {"oracle": 0, "model": 0}
    for n, B in cases():
        for xs, ys in operand_shapes(op, n, B):
            x = dense((B,) + xs, 1000 * n[0] + n[1] + B)
            y = dense((B,) + ys, 2000 * n[0] + n[1] + B + 7)
            if oracle_is_normative(op, x, y):
                expect, by = want(oracle_lib, OTP, op, x, y, n), "oracle"
            else:  # a divisor / operand of log with a single row or column: small items only (operand_shapes)
                assert n[0] * n[1] <= 64
                expect, by = model_batch(op, x, y, n), "model"
            got = run(op, x, y, n)
            assert_bits(got, expect, f"{op} n={n} B={B} x{xs} y{ys} against the {by}")
            checked[by] += 1
    assert checked["oracle"] >= 30 and (checked["model"] > 0) == (op in ("div", "log"))


@pytest.mark.parametrize("op", ["div", "log"])
def test_model_cases(op):
    """divisors / operands of log with a length-1 axis, where the reference shortcuts or stores fewer rows: the loops of
    include/gftaylor.h are the definition"""
    for n in [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (8, 8)]:
        for ts in {(1, n[1]), (n[0], 1), (1, 1)}:
            B = 3
            if op == "div":
                x, y = dense((B,) + n, 31 * n[0] + n[1]), dense((B,) + ts, 37 * n[0] + n[1])
            else:
                x, y = dense((B,) + ts, 41 * n[0] + n[1]), None
            got = run(op, x, y, n)
            assert_bits(got, model_batch(op, x, y if y is not None else x, n), f"{op} n={n} operand {ts}")


# ---- device seeds ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,B", [((8, 8), 300), ((5, 64), 3), ((16, 16), 65)])
def test_device_seeds(n, B, OTP):
    x = dense((B,) + n, 31 * n[0] + B)
    for op in ("exp", "log"):
        expect = want_handle(OTP, op, x, None, n)
        got = run(op, x, None, n, seed=None).cpu().numpy()
        if op == "log":  # only coefficient [0, 0] depends on the seed
            g, w = got.copy(), expect.copy()
            g[:, 0, 0] = w[:, 0, 0] = 0.0
            assert_bits(g, w, f"log n={n} B={B} device seed, all but [0, 0]")
            got, expect = got[:, :1, :1], expect[:, :1, :1]
        assert np.all(np.abs(got - expect) <= REL_TOL * np.abs(expect)), (op, n, B, np.max(np.abs(got - expect) / np.abs(expect)))


# ---- views -----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,batch", [((3, 5), (4, 5)), ((9, 65), (2, 3)), ((16, 16), (7,))])
def test_views(n, batch, OTP, oracle_lib):
    from genfer_amd import series2

    B, nb = int(np.prod(batch)), len(batch)
    x, y = dense((B,) + n, 11), dense((B,) + n, 12)
    expect = {op: want(oracle_lib, OTP, op, x, y, n).reshape(batch + n) for op in OPS}
    X, Y = dev(x).reshape(batch + n), dev(y).reshape(batch + n)
    seeds = {op: dev(host_seeds(op, x)).reshape(batch) for op in ("exp", "log")}

    def call(op, a, b, **kw):
        return getattr(series2, op)(a, b, **kw) if op in ("mul", "div") else getattr(series2, op)(a, seed=seeds[op], **kw)

    # a row-strided operand: a slice of a wider tensor on both series axes
    wide = torch.zeros(batch + (n[0] + 3, n[1] + 9), dtype=torch.float64, device=DEV)
    wide[..., 1:1 + n[0], 4:4 + n[1]] = X
    xs = wide[..., 1:1 + n[0], 4:4 + n[1]]
    assert not xs.is_contiguous() and xs.stride(-2) == n[1] + 9
    for op in OPS:
        assert_bits(call(op, xs, Y), expect[op], f"{op} sliced x")
    # a transposed batch
    if nb >= 2:
        perm = tuple(reversed(range(nb))) + (nb, nb + 1)
        xp = X.permute(*perm).contiguous().permute(*perm)
        assert not xp.is_contiguous() and xp.stride(-1) == 1
        for op in OPS:
            assert_bits(call(op, xp, Y), expect[op], f"{op} permuted x")
        po = torch.empty(tuple(reversed(batch)) + n, dtype=torch.float64, device=DEV).permute(*perm)
        series2.div(X, Y, out=po)
        assert_bits(po, expect["div"], "div permuted out")
    # an out= view with guard words around it, intact afterwards
    for op in OPS:
        big = torch.full(batch + (n[0] + 2, n[1] + 5), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
        out = big[..., 1:1 + n[0], 2:2 + n[1]]
        assert call(op, xs, Y, out=out) is out
        assert_bits(out, expect[op], f"{op} sliced out")
        g = big.view(torch.int64).clone()
        g[..., 1:1 + n[0], 2:2 + n[1]] = GUARD
        assert bool((g == GUARD).all()), op
    # batch stride 0: one item against the batch, on either side, and a row repeated inside an item
    y0 = np.repeat(y[:1], B, axis=0)
    ye = dev(y[:1]).reshape((1,) * nb + n).expand(batch + n)
    assert ye.stride(0) == 0
    assert_bits(series2.mul(X, ye), want(oracle_lib, OTP, "mul", x, y0, n).reshape(batch + n), "mul expanded y")
    assert_bits(series2.div(X, dev(y[0])), want(oracle_lib, OTP, "div", x, y0, n).reshape(batch + n), "div broadcast y")
    assert_bits(series2.div(ye, X), want(oracle_lib, OTP, "div", y0, x, n).reshape(batch + n), "div expanded x")
    xrow = np.repeat(x[:, :1], n[0], axis=1)  # every row of an item the same row: row stride 0
    xr = dev(x[:, :1]).reshape(batch + (1, n[1])).expand(batch + n)
    assert xr.stride(-2) == 0
    assert_bits(series2.mul(xr, Y), want(oracle_lib, OTP, "mul", xrow, y, n).reshape(batch + n), "mul with a row stride of 0")
    # in place
    for op in OPS:
        xi = X.clone()
        assert call(op, xi, Y, out=xi) is xi
        assert_bits(xi, expect[op], f"{op} in place on x")
    for op in ("mul", "div"):
        yi = Y.clone()
        call(op, X, yi, out=yi)
        assert_bits(yi, expect[op], f"{op} in place on y")
        wi = wide.clone()  # in place on a strided view
        v = wi[..., 1:1 + n[0], 4:4 + n[1]]
        call(op, v, Y, out=v)
        assert_bits(v, expect[op], f"{op} in place on a sliced x")


def test_compact_operands_and_explicit_orders(oracle_lib, OTP):
    """n defaults to the larger stored length on each axis, and may be larger than both operands"""
    from genfer_amd import series2

    x, y = dense((5, 3, 6), 61), dense((5, 4, 2), 62)
    assert_bits(series2.mul(dev(x), dev(y)), want(oracle_lib, OTP, "mul", x, y, (4, 6)), "mul default n")
    assert_bits(series2.mul(dev(x), dev(y), n=(9, 11)), want(oracle_lib, OTP, "mul", x, y, (9, 11)), "mul n beyond both")
    assert_bits(series2.div(dev(x), dev(y), n=(7, 9)), want(oracle_lib, OTP, "div", x, y, (7, 9)), "div n beyond both")
    assert_bits(run("exp", x, None, (6, 9)), want(oracle_lib, OTP, "exp", x, None, (6, 9)), "exp n beyond x")
    assert_bits(run("log", x, None, (6, 9)), want(oracle_lib, OTP, "log", x, None, (6, 9)), "log n beyond x")


def test_empty_batch_is_a_no_op():
    from genfer_amd import series2

    e = torch.zeros((0, 3, 8), dtype=torch.float64, device=DEV)
    assert series2.mul(e, e).shape == (0, 3, 8) and series2.exp(e).shape == (0, 3, 8)


# ---- special values ----------------------------------------------------------------------------------------------------------------

INF, NAN = float("inf"), float("nan")


def test_special_values():
    """infinities, NaNs, exact zeros and negative zeros follow the definition bit for bit (a NaN for a NaN); only stored
    coefficients enter a sum, so a compact operand next to an infinity leaves the coefficients it does not reach finite; and an
    item does not change its neighbour in the batch"""
    from genfer_amd import series2

    n = (4, 5)
    plain = dense(n, 71)
    items = []
    for (i, j, v) in [(1, 1, INF), (0, 2, -INF), (2, 0, NAN), (1, 3, INF)]:
        a = plain.copy()
        a[i, j] = v
        items.append(a)
    z = plain.copy()
    z[1:, :] = 0.0
    z[0, 2:] = -0.0
    items += [z, -z, np.where(np.eye(*n) > 0, 1.0, np.where(plain > 1.0, -0.0, 0.0)), plain]
    x = np.stack(items)
    x[:, 0, 0] = np.abs(plain[0, 0])  # seeds the host libm can form, divisors with y[0, 0] != 0
    y = np.stack(items[::-1])
    y[:, 0, 0] = 1.25
    with np.errstate(all="ignore"):
        for op in OPS:
            got = run(op, x, y, n)
            assert_bits(got, model_batch(op, x, y, n), f"{op} specials")
            alone = run(op, x[-1:], y[-1:], n)
            assert torch.equal(bits(alone), bits(got[-1:])), (op, "the plain item inside the batch of specials")
        # a zero divisor coefficient [0, 0]: the definition divides by it
        y0 = y.copy()
        y0[:, 0, 0] = [0.0, -0.0, 0.0, INF, NAN, 0.0, -0.0, 1.0]
        assert_bits(run("div", x, y0, n), model_batch("div", x, y0, n), "div by y[0, 0] in {0, -0, inf, nan}")
        # compact x of (2, 2) with an infinity in its corner: it reaches the outputs (k0 >= 1, k1 >= 1) only
        xc = dense((3, 2, 2), 72)
        xc[:, 1, 1] = INF
        yd = dense((3,) + n, 73)
        got = series2.mul(dev(xc), dev(yd), n=n).cpu().numpy()
        assert_bits(got, model_batch("mul", xc, yd, n), "mul compact x with an infinity")
        assert np.isfinite(got[:, 0, :]).all() and np.isfinite(got[:, :, 0]).all() and np.isinf(got[:, 1:, 1:]).all()
        got = series2.div(dev(xc), dev(yd), n=n).cpu().numpy()
        assert_bits(got, model_batch("div", xc, yd, n), "div compact x with an infinity")
        assert np.isfinite(got[:, 0, :]).all() and np.isfinite(got[:, :, 0]).all() and not np.isfinite(got[:, 1:, 1:]).any()


# ---- refusals and limits -----------------------------------------------------------------------------------------------------------


def test_refusals_and_limits():
    from genfer_amd import series, series2
    from genfer_amd.taylor import TaylorError

    x = torch.rand((6, 4, 16), dtype=torch.float64, device=DEV) + 0.5
    y = torch.rand((6, 4, 16), dtype=torch.float64, device=DEV) + 0.5

    def after():  # no stale HIP error: torch's next call succeeds
        assert float((x + 1.0).sum().item()) > 0

    with pytest.raises(TaylorError, match="unit stride"):
        series2.mul(torch.rand((6, 4, 32), dtype=torch.float64, device=DEV)[..., ::2], y)
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series2.mul(x, y, n=(17, 241))  # 4097
    after()
    with pytest.raises(TaylorError, match="nx > n"):
        series2.mul(x, y, n=(4, 8))
    with pytest.raises(TaylorError, match="float32"):
        series2.mul(x.float(), y)
    with pytest.raises(TaylorError, match="on cpu"):
        series2.mul(x.cpu(), y)
    with pytest.raises(TaylorError, match="no autograd"):
        series2.mul(x.clone().requires_grad_(), y)
    with pytest.raises(TaylorError, match="zero stride"):
        series2.mul(x, y, out=torch.empty((1, 4, 16), dtype=torch.float64, device=DEV).expand(6, 4, 16))
    after()
    with pytest.raises(TaylorError, match="zero row stride"):
        series2.mul(x, y, out=torch.empty((6, 1, 16), dtype=torch.float64, device=DEV).expand(6, 4, 16))
    after()
    with pytest.raises(TaylorError, match="overlap"):  # rows 8 apart, 16 long: the result's rows overlap each other
        series2.mul(x, y, out=torch.empty(1024, dtype=torch.float64, device=DEV).as_strided((6, 4, 16), (64, 8, 1)))
    after()
    # a partial overlap with an operand is refused, by address range
    buf = torch.rand((6, 4, 40), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps x"):
        series2.mul(buf[..., 0:16], y, out=buf[..., 8:24])
    with pytest.raises(TaylorError, match="partially overlaps y"):
        series2.div(x, buf[:, :, 0:16], out=buf[:, :, 16:32])  # interleaved rows of one buffer
    rows = torch.rand((6, 8, 16), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps x"):
        series2.exp(rows[:, 0:4], out=rows[:, 2:6])
    sd = torch.rand((6, 4, 16), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps the seeds"):
        series2.exp(x, seed=sd[:, 0, 0], out=sd)
    after()
    # through the C entry points: the limit, an empty result, an operand longer than the result, a negative row stride
    series2.mul(x, y)  # declares the entry points
    import genfer_amd

    L = genfer_amd.lib()
    one = (C.c_size_t * 1)(6)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    big = torch.zeros(6 * 4097, dtype=torch.float64, device=DEV)

    def c_mul(nx, ny, nr, rrs=None):
        return L.gft_series2_mul(vp(x), None, 16, nx[0], nx[1], vp(y), None, 16, ny[0], ny[1], vp(big), None, nr[1] if rrs is None else rrs,
                                 nr[0], nr[1], one, 1, None)

    assert c_mul((4, 16), (4, 16), (17, 241)) == -1
    assert "n0 * n1 = 17 * 241 exceeds the limit of 4096" in L.gft_last_error().decode()
    assert c_mul((4, 16), (4, 16), (0, 16)) == -1 and "n0 * n1 == 0" in L.gft_last_error().decode()
    assert c_mul((4, 16), (4, 16), (3, 16)) == -1 and "x has 4 x 16 coefficients, the result 3 x 16" in L.gft_last_error().decode()
    assert c_mul((4, 16), (4, 16), (4, 16), rrs=-16) == -1 and "negative strides" in L.gft_last_error().decode()
    assert c_mul((4, 16), (4, 16), (4, 16)) == 0
    after()
    # the limit itself runs (both ways), and the calls after the refusals are unharmed
    for n in [(64, 64), (1, 4096), (4096, 1)]:
        a = torch.rand((2,) + n, dtype=torch.float64, device=DEV) + 0.5
        assert series2.mul(a, a).shape == (2,) + n and series.last_form() == "B"
    assert torch.equal(bits(series2.mul(x, y)), bits(series2.mul(x.clone(), y.clone())))


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


@pytest.mark.parametrize("which", ["side_stream", "null_stream"])
def test_stream_ordered_without_host_stall(which, oracle_lib, OTP):
    from genfer_amd import series2

    B, n = 512, (4, 6)
    x, y = dense((B,) + n, 41), dense((B,) + n, 42)
    expect = want(oracle_lib, OTP, "mul", x, y, n)
    X, Y = dev(x), dev(y)
    src = torch.zeros((B,) + n, dtype=torch.float64, device=DEV)
    series2.mul(src, Y)  # warm the kernel
    cycles = _sleep_cycles_for_ms(100)
    s = torch.cuda.Stream() if which == "side_stream" else torch.cuda.default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        src.copy_(X)  # the operand is produced behind a long kernel on this stream
        z = series2.mul(src, Y)
        done = torch.cuda.Event()
        done.record()
        returned_early = not done.query()  # allowed to be false, never required
        twice = z * 2.0  # consumed right after, no host synchronisation in between
        src.zero_()  # the operand is reused right after
    s.synchronize()
    assert_bits(z, expect, "mul on " + which)
    assert_bits(twice, expect * 2.0, "consumer on " + which)
    assert returned_early in (True, False)
