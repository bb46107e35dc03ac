"""Batched univariate series on device tensors (genfer_amd.series, gft_series_mul / div / exp / log) on the MI355X.

Every coefficient of every item carries the oracle's bits (the reference's general algorithms in its order), in both forms
of the kernels and on every side of the dispatch; views, broadcasting, in-place results, refusals and the stream contract."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import REL_TOL, splitmix64_uniform

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield
    genfer_amd.series.set_form(None)


@pytest.fixture(autouse=True)
def _auto_form():
    from genfer_amd import series

    series.set_form(None)
    yield
    series.set_form(None)


# ---- expected values: the CPU oracle, one item at a time -------------------------------------------------------------------


def dense(shape, seed):
    """0.5 + uniform: dense rows, divisors neither constant nor one — the oracle takes no shortcut"""
    return (0.5 + splitmix64_uniform(seed, int(np.prod(shape)))).reshape(shape)


def pad(a, n):
    out = np.zeros(n)
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    out[:a.size] = a
    return out


def want_mul(oracle_lib, x, y, n):
    """orc_mul_raw on a zeroed result: the general product, no dispatcher"""
    szp = C.POINTER(C.c_size_t)
    oracle_lib.orc_mul_raw.restype = C.c_int
    oracle_lib.orc_mul_raw.argtypes = [C.c_void_p, szp, C.c_void_p, szp, C.c_void_p, szp, C.c_size_t]
    out = np.zeros((x.shape[0], n))
    one = lambda v: (C.c_size_t * 1)(v)  # noqa: E731
    for b in range(x.shape[0]):
        xr, yr = np.ascontiguousarray(x[b]), np.ascontiguousarray(y[b])
        oracle_lib.orc_mul_raw(xr.ctypes.data_as(C.c_void_p), one(xr.size), yr.ctypes.data_as(C.c_void_p), one(yr.size),
                               out[b].ctypes.data_as(C.c_void_p), one(n), 1)
    return out


def want_handle(OTP, op, x, y, n):
    """div / exp / log through the oracle's handle API (platform libm seeds)"""
    out = np.zeros((x.shape[0], n))
    for b in range(x.shape[0]):
        p = OTP.new(x[b], (n,))
        r = p / OTP.new(y[b], (n,)) if op == "div" else (p.exp() if op == "exp" else p.log())
        out[b] = pad(r.array(), n)
    return out


def host_seeds(op, x):
    f = math.exp if op == "exp" else math.log
    return np.array([f(v) for v in x[:, 0]])


def assert_bits(got, want, what):
    """every bit of every coefficient; where the oracle's value is NaN, a NaN (the convention of the reference-order tests)"""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    ok = np.where(nan, np.isnan(got), got.view(np.int64) == want.view(np.int64))
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {(~ok).sum()} coefficients differ, first at {i}: got {got[i]!r} want {want[i]!r}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(op, x, y, n, form=None, seed="host"):
    """x, y: numpy [B, nx] / [B, ny]; the batched call in the asked form, and the form that ran"""
    from genfer_amd import series

    series.set_form(form)
    tx = dev(x)
    if op in ("mul", "div"):
        got = getattr(series, op)(tx, dev(y), n=n)
    else:
        sd = dev(host_seeds(op, x)) if seed == "host" else None
        got = getattr(series, op)(tx, n=n, seed=sd)
    ran = series.last_form()
    series.set_form(None)
    return got, ran


# ---- bit-exact against the oracle, per item, both forms, every side of the dispatch ---------------------------------------------

ORDERS = [1, 2, 3, 7, 16, 31, 32, 33, 64, 65, 100, 257, 1024, 4096]
BATCHES = [1, 3, 64, 65, 1000]
CPU_BUDGET = 7.0e7  # B * n^2 per case: the oracle side stays within seconds


def cases():
    for n in ORDERS:
        for B in BATCHES:
            if B > 3 and B * n * n > CPU_BUDGET:
                continue  # a handful of rows at the big orders
            yield n, B


def lengths(op, n, B):
    """(nx, ny): dense, and compact operands (nx < n, ny < n, nx = 1) on some of the batches; the divisor of div and the
    operand of exp / log keep at least two coefficients, so the oracle takes its general path"""
    out = [(n, n)]
    if n >= 3 and B in (3, 65):
        out += [(n // 2, n - 1), (1, max(2, n // 3) if op == "mul" else n)]
    return out


@pytest.mark.parametrize("op", ["mul", "div", "exp", "log"])
def test_bit_exact_against_the_oracle(op, OTP, oracle_lib):
    seen = {}
    for n, B in cases():
        for nx, ny in lengths(op, n, B):
            x, y = dense((B, nx), 1000 * n + B), dense((B, ny), 2000 * n + B + 7)
            want = want_mul(oracle_lib, x, y, n) if op == "mul" else want_handle(OTP, op, x, y, n)
            forms = set()
            for form in (None, "A", "B"):
                got, ran = run(op, x, y, n, form)
                assert ran in ("A", "B")
                if form == "B":
                    assert ran == "B"
                assert_bits(got, want, f"{op} n={n} B={B} nx={nx} ny={ny} form={ran}")
                forms.add(ran)
                seen.setdefault(ran, []).append((n, B))
            if n <= 63:
                assert forms == {"A", "B"}, (n, B, forms)  # short rows fit form A: both forms were compared
            if n > 79:
                assert forms == {"B"}, (n, B, forms)
    # both forms ran, and the dispatch itself chose each of them somewhere
    assert seen.get("A") and seen.get("B")


@pytest.mark.parametrize("op", ["mul", "div"])
def test_dispatch_by_batch_size(op):
    """the thresholds themselves: short rows take form A from 256 items on, form B below; long rows always form B"""
    from genfer_amd import series

    for n, B, want in [(16, 1000, "A"), (16, 65, "B"), (48, 256, "A"), (48, 255, "B"), (100, 1000, "B"), (32, 3, "B")]:
        x, y = dev(dense((B, n), 5)), dev(dense((B, n), 6))
        getattr(series, op)(x, y)
        assert series.last_form() == want, (n, B)
    series.exp(dev(dense((3, 32), 5)))
    assert series.last_form() == "A"
    series.log(dev(dense((3, 128), 5)))
    assert series.last_form() == "B"


# ---- device seeds --------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,B", [(16, 1000), (64, 65), (100, 3), (300, 64)])
def test_device_seeds(n, B, OTP):
    x = dense((B, n), 31 * n + B)
    for op in ("exp", "log"):
        want = want_handle(OTP, op, x, None, n)
        got = run(op, x, None, n, seed=None)[0].cpu().numpy()
        if op == "log":  # only coefficient 0 depends on the seed
            assert_bits(got[:, 1:], want[:, 1:], f"log n={n} B={B} device seed, k >= 1")
            got, want = got[:, :1], want[:, :1]
        assert np.all(np.abs(got - want) <= REL_TOL * np.abs(want)), (op, n, B, np.max(np.abs(got - want) / np.abs(want)))


# ---- special values ------------------------------------------------------------------------------------------------------------

INF, NAN = float("inf"), float("nan")
TINY, HUGE = 5e-324, 1.7e308


def special_rows(n):
    rows = [
        [0.0] * n, [-0.0] * n, [1.0] + [0.0] * (n - 1), [2.5] + [0.0] * (n - 1), [-0.0, 1.0] + [0.0] * (n - 2),
        [TINY] * n, [2.2e-308, -TINY] * (n // 2), [HUGE, -HUGE] * (n // 2), [1e-200] * n, [1e200] * n,
        [1.0, INF] + [1.0] * (n - 2), [1.0, -INF, INF] + [0.5] * (n - 3), [1.0, NAN] + [1.0] * (n - 2),
        [0.0, 1.0, 2.0] + [1.0] * (n - 3), [-1.5, 0.25] * (n // 2),
    ]
    return np.array(rows, dtype=np.float64)


@pytest.mark.parametrize("form", ["A", "B"])
def test_special_values(form, OTP, oracle_lib):
    n = 8
    rows = special_rows(n)
    R = rows.shape[0]
    x = np.repeat(rows, R, axis=0)  # every row against every row
    y = np.tile(rows, (R, 1))
    with np.errstate(all="ignore"):
        got, ran = run("mul", x, y, n, form)
        assert ran == form
        assert_bits(got, want_mul(oracle_lib, x, y, n), f"mul specials form {form}")
        # div: the general recurrence restated in the reference's order (_np_div): the oracle's operator shortcuts on a constant
        # divisor, which the batch must not; y[0] = 0, +-inf and NaN divisors included
        want = _np_div(x, y, n)
        got, ran = run("div", x, y, n, form)
        assert ran == form
        assert_bits(got, want, f"div specials form {form}")
        # ... and the oracle itself wherever it takes the general path (a dense divisor)
        dense_y = np.array([not (np.all(r[1:] == 0)) for r in y])
        wo = want_handle(OTP, "div", x[dense_y], y[dense_y], n)
        assert_bits(got.cpu().numpy()[dense_y], wo, f"div specials vs the oracle, form {form}")
        for op in ("exp", "log"):
            x0 = rows[:, 0]  # seeds the host libm can form
            xs = rows[(np.abs(x0) < 700) if op == "exp" else (np.isfinite(x0) & (x0 > 0))]
            got, ran = run(op, xs, None, n, form)
            assert ran == form
            assert_bits(got, want_handle(OTP, op, xs, None, n), f"{op} specials form {form}")


def _np_div(x, y, n):
    with np.errstate(all="ignore"):
        want = np.zeros((x.shape[0], n))
        for b in range(x.shape[0]):
            for k in range(n):
                s = 0.0
                for j in range(k):
                    s = s + want[b, j] * y[b, k - j]
                want[b, k] = (-s + x[b, k]) / y[b, 0]
    return want


@pytest.mark.parametrize("n,B", [(8, 300), (8, 5), (96, 5)])
def test_no_shortcuts_and_no_neighbours(n, B, oracle_lib):
    """rows on which the operator wrappers would shortcut get the general recurrence, alone and inside a dense batch"""
    from genfer_amd import series

    x, y = dense((B, n), 77), dense((B, n), 78)
    x[0] = 0.0  # zero operand
    y[1] = [3.0] + [0.0] * (n - 1)  # constant divisor
    y[2] = [1.0] + [0.0] * (n - 1)  # y = 1
    x[3] = [2.0] + [0.0] * (n - 1)  # constant operand
    x[4] = [1.0, 0.5] + [0.0] * (n - 2)  # linear operand
    assert_bits(series.mul(dev(x), dev(y)), want_mul(oracle_lib, x, y, n), "mul with shortcut rows")
    q = series.div(dev(x), dev(y))
    assert_bits(q, _np_div(x, y, n), "div with shortcut rows")
    for b in range(5):  # each row alone == the row in the batch
        for op in ("mul", "div"):
            alone = getattr(series, op)(dev(x[b:b + 1]), dev(y[b:b + 1]))
            batch = getattr(series, op)(dev(x), dev(y))
            assert torch.equal(alone.view(torch.int64), batch[b:b + 1].contiguous().view(torch.int64)), (op, b)


# ---- views -----------------------------------------------------------------------------------------------------------------------


def bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("n,batch", [(12, (5, 70)), (40, (3, 4, 6)), (130, (2, 5)), (20, (7,))])
def test_views(n, batch, oracle_lib):
    from genfer_amd import series

    B = int(np.prod(batch))
    x, y = dense((B, n), 11), dense((B, n), 12)
    wm = want_mul(oracle_lib, x, y, n).reshape(batch + (n,))
    wd = _np_div(x, y, n).reshape(batch + (n,))
    X, Y = dev(x).reshape(batch + (n,)), dev(y).reshape(batch + (n,))
    # slices of wider tensors
    wide = torch.zeros(batch + (n + 9,), dtype=torch.float64, device=DEV)
    wide[..., 4:4 + n] = X
    xs = wide[..., 4:4 + n]
    assert not xs.is_contiguous()
    assert_bits(series.mul(xs, Y), wm, "sliced x")
    assert_bits(series.div(xs, Y), wd, "sliced x")
    # batch axes permuted
    if len(batch) >= 2:
        perm = tuple(reversed(range(len(batch))))
        yp = Y.permute(*perm, len(batch)).contiguous().permute(*perm, len(batch))
        assert not yp.is_contiguous() and yp.stride(-1) == 1
        assert_bits(series.mul(X, yp), wm, "permuted y")
        assert_bits(series.div(X, yp), wd, "permuted y")
    # a sliced out with guards around it, untouched
    big = torch.full(batch + (n + 5,), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
    out = big[..., 2:2 + n]
    assert series.mul(xs, Y, out=out) is out
    assert_bits(out, wm, "sliced out")
    g = big.view(torch.int64)
    assert bool((g[..., :2] == GUARD).all()) and bool((g[..., 2 + n:] == GUARD).all())
    # out with permuted batch axes
    if len(batch) >= 2:
        po = torch.empty(tuple(reversed(batch)) + (n,), dtype=torch.float64, device=DEV).permute(*perm, len(batch))
        series.div(X, Y, out=po)
        assert_bits(po, wd, "permuted out")
    # one series against the batch (stride 0), on either side
    y0 = y[:1]
    yb = np.repeat(y0, B, axis=0)
    ye = dev(y0).reshape((1,) * len(batch) + (n,)).expand(batch + (n,))
    assert ye.stride()[0] == 0
    assert_bits(series.mul(X, ye), want_mul(oracle_lib, x, yb, n).reshape(batch + (n,)), "expanded y")
    assert_bits(series.div(X, dev(y0)[0]), _np_div(x, yb, n).reshape(batch + (n,)), "broadcast 1-d y")
    assert_bits(series.div(ye, X), _np_div(yb, x, n).reshape(batch + (n,)), "expanded x")
    assert_bits(series.mul(dev(y0)[0], X), want_mul(oracle_lib, yb, x, n).reshape(batch + (n,)), "broadcast 1-d x")
    # in place
    for form in ("A", "B"):
        series.set_form(form)
        xi = X.clone()
        assert series.mul(xi, Y, out=xi) is xi
        assert_bits(xi, wm, f"mul in place, form {form}")
        xi = X.clone()
        series.div(xi, Y, out=xi)
        assert_bits(xi, wd, f"div in place, form {form}")
        yi = Y.clone()
        series.div(X, yi, out=yi)
        assert_bits(yi, wd, f"div in place on the divisor, form {form}")
    series.set_form(None)


@pytest.mark.parametrize("n,batch", [(12, (5, 70)), (130, (2, 5))])
def test_views_exp_log(n, batch, OTP):
    from genfer_amd import series

    B = int(np.prod(batch))
    x = dense((B, n), 21)
    X = dev(x).reshape(batch + (n,))
    for op in ("exp", "log"):
        want = want_handle(OTP, op, x, None, n).reshape(batch + (n,))
        sd = dev(host_seeds(op, x)).reshape(batch)
        f = getattr(series, op)
        perm = tuple(reversed(range(len(batch))))
        xp = X.permute(*perm, len(batch)).contiguous().permute(*perm, len(batch))
        sp = sd.permute(*perm).contiguous().permute(*perm)
        assert_bits(f(xp, seed=sp), want, f"{op} permuted")
        big = torch.full(batch + (n + 5,), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
        out = big[..., 2:2 + n]
        f(X, seed=sd, out=out)
        assert_bits(out, want, f"{op} sliced out")
        g = big.view(torch.int64)
        assert bool((g[..., :2] == GUARD).all()) and bool((g[..., 2 + n:] == GUARD).all())
        xi = X.clone()
        f(xi, seed=sd, out=xi)
        assert_bits(xi, want, f"{op} in place")
        # one series for the whole batch
        xe = X[(0,) * len(batch)].expand(batch + (n,))
        se = sd[(0,) * len(batch)].expand(batch)
        assert_bits(f(xe, seed=se), np.broadcast_to(want[(0,) * len(batch)], batch + (n,)).copy(), f"{op} expanded")


def test_empty_batch_is_a_no_op():
    from genfer_amd import series

    z = series.mul(torch.zeros((0, 8), dtype=torch.float64, device=DEV), torch.zeros((0, 8), dtype=torch.float64, device=DEV))
    assert z.shape == (0, 8)


# ---- refusals --------------------------------------------------------------------------------------------------------------------


def test_refusals_name_the_cause():
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    x = torch.rand((6, 16), dtype=torch.float64, device=DEV)
    y = torch.rand((6, 16), dtype=torch.float64, device=DEV)

    def after():  # no stale HIP error: torch's next call succeeds
        assert float((x + 1.0).sum().item()) > 0

    with pytest.raises(TaylorError, match="unit stride"):
        series.mul(torch.rand((6, 32), dtype=torch.float64, device=DEV)[:, ::2], y)
    after()
    with pytest.raises(TaylorError, match="4096"):
        series.mul(x, y, n=4097)
    after()
    with pytest.raises(TaylorError, match="nx > n"):
        series.mul(x, y, n=8)
    after()
    with pytest.raises(TaylorError, match="float32"):
        series.mul(x.float(), y)
    after()
    with pytest.raises(TaylorError, match="on cpu"):
        series.mul(x.cpu(), y)
    after()
    with pytest.raises(TaylorError, match="zero stride"):
        series.mul(x, y, out=torch.empty((1, 16), dtype=torch.float64, device=DEV).expand(6, 16))
    after()
    buf = torch.rand((6, 40), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps x"):
        series.mul(buf[:, 0:16], y, out=buf[:, 8:24])
    after()
    with pytest.raises(TaylorError, match="overlap"):
        series.mul(x, y, out=torch.empty(64, dtype=torch.float64, device=DEV).as_strided((6, 16), (4, 1)))
    after()
    # through the C entry points: n == 0, nx > n
    L = genfer_lib()
    one = (C.c_size_t * 1)(6)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.gft_series_mul(vp(x), None, 16, vp(y), None, 16, vp(y), None, 0, one, 1, None) == -1
    assert "n == 0" in L.gft_last_error().decode()
    assert L.gft_series_mul(vp(x), None, 16, vp(y), None, 4, vp(y), None, 8, one, 1, None) == -1
    assert "nx = 16 > n = 8" in L.gft_last_error().decode()
    assert L.gft_series_exp(vp(x), None, 16, None, None, vp(y), None, 4097, one, 1, None) == -1
    assert "4096" in L.gft_last_error().decode()
    after()
    assert_bits(series.mul(x, y), series.mul(x.clone(), y.clone()).cpu().numpy(), "after the refusals")


def genfer_lib():
    import genfer_amd
    from genfer_amd import series

    series.last_form()  # declares the entry points
    return genfer_amd.lib()


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
def test_stream_ordered_without_host_stall(which, oracle_lib):
    from genfer_amd import series

    B, n = 512, 24
    x, y = dense((B, n), 41), dense((B, n), 42)
    want = want_mul(oracle_lib, x, y, n)
    X, Y = dev(x), dev(y)
    src = torch.zeros((B, n), dtype=torch.float64, device=DEV)
    series.mul(src, Y)  # warm the kernel
    cycles = _sleep_cycles_for_ms(100)
    s = torch.cuda.Stream() if which == "side_stream" else torch.cuda.default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        src.copy_(X)  # the operand is produced behind a long kernel on this stream
        z = series.mul(src, Y)
        done = torch.cuda.Event()
        done.record()
        returned_early = not done.query()  # allowed to be false, never required
        twice = z * 2.0  # consumed right after, no host synchronisation in between
        src.zero_()  # the operand is reused right after
    s.synchronize()
    assert_bits(z, want, "mul on " + which)
    assert_bits(twice, want * 2.0, "consumer on " + which)
    assert returned_early in (True, False)


# ---- the handle API computes the same bits on the device ---------------------------------------------------------------------------


def test_agrees_with_the_handle_api():
    import genfer_amd
    from genfer_amd import series

    TP = genfer_amd.TaylorPoly
    B, n = 6, 48
    x, y = dense((B, n), 51), dense((B, n), 52)
    X, Y = dev(x), dev(y)
    assert genfer_amd.lib().gft_set_conv_mode(3) == 0  # reference order
    try:
        zm, zd = series.mul(X, Y), series.div(X, Y)
        ze = series.exp(X, seed=dev(host_seeds("exp", x)))
        zl = series.log(X, seed=dev(host_seeds("log", x)))
        for b in range(B):
            p, q = TP.from_torch(X[b]), TP.from_torch(Y[b])
            assert torch.equal(bits(zm[b]), bits((p * q).to_torch())), b
            assert torch.equal(bits(zd[b]), bits((p / q).to_torch())), b
            assert torch.equal(bits(ze[b]), bits(p.exp().to_torch())), b
            assert torch.equal(bits(zl[b]), bits(p.log().to_torch())), b
    finally:
        assert genfer_amd.lib().gft_set_conv_mode(0) == 0
