"""Batched BigFloat series on device tensors (genfer_amd.bigfloat_series, gftb_series_*) on the MI355X.

Every factor and exponent of every coefficient of every item carries the oracle's bits (a NaN factor only has to be a NaN), in both
forms of the kernels and on both sides of every dispatch boundary of two-plane rows, on rows whose values leave the f64 range, on
rows that meet the tiny-term drop of 0 + b, and on rows with infinities and NaNs; every layout (broadcast, slices, a transposed batch,
planes from separate allocations, out= with guard words, in place), the refusals, the stream contract, device seeds and the round
trip through encode / decode against series.mul.  The data, the cases and the expected values come from
tests/test_bigfloat_series_cpu.py, which checks them against each other and for sanity without a GPU."""
import ctypes as C

import numpy as np
import pytest

from conftest import REL_TOL
from test_bigfloat_series_cpu import (FINITE, KINDS, OPS, OTPB, bit_exact_cases, crafted, data, expected, host_seeds, operands, orcb,  # noqa: F401
                                      want_compose, want_handle, want_mul, want_pow)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 0x5A5A5A5A5A5A5A5A
FORM_A_MAX = {"mul": 39, "div": 39, "exp": 39, "log": 39, "compose": 25, "pow": 39}  # gft_series.hip: 2 (3) arrays of two planes in 80 KB
FORM_A_MAX_PLAIN = {"mul": 31, "div": 31, "exp": 31, "log": 31, "compose": 21, "pow": 31}  # where the runtime grants 64 KB only


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield
    genfer_amd.bigfloat_series.set_form(None)


@pytest.fixture(autouse=True)
def _auto_form():
    from genfer_amd import bigfloat_series as bfs

    bfs.set_form(None)
    yield
    bfs.set_form(None)


def assert_bits(got, want, what):
    """every bit of every factor and exponent; where the oracle's factor is a NaN, a NaN (tests/test_bigfloat_gpu.py's rule) -- its
    exponent, a finite number, is compared exactly like everything else"""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    want = np.ascontiguousarray(want).reshape(got.shape)
    got = np.ascontiguousarray(got)
    nan = np.isnan(want)
    assert not nan[1].any(), what  # (no expected exponent is a NaN)
    ok = np.where(nan, np.isnan(got), got.view(np.int64) == want.view(np.int64))
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {(~ok).sum()} of {ok.size} values differ, first at {i}: got {got[i]!r} want {want[i]!r} "
                             f"(factor {got[(0,) + i[1:]]!r} exponent {got[(1,) + i[1:]]!r}; want {want[(0,) + i[1:]]!r}, {want[(1,) + i[1:]]!r})")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64)


def call(op, x, y=None, n=None, out=None, seeds=None, e=3):
    from genfer_amd import bigfloat_series as bfs

    if op in ("mul", "div", "compose"):
        return getattr(bfs, op)(x, y, n=n, out=out)
    if op == "pow":
        return bfs.pow(x, e, n=n, out=out)
    return getattr(bfs, op)(x, n=n, seed=seeds, out=out)


def run(op, X, Y, n, form=None, seeds=None, e=None, batch=None):
    """X, Y: numpy [2, B, nx] / [2, B, ny] (reshaped to the batch axes `batch`); the call in the asked form, and the form that ran"""
    from genfer_amd import bigfloat_series as bfs

    def shaped(a, tail):
        return None if a is None else dev(a).reshape((2,) + (batch or (a.shape[1],)) + tail)

    bfs.set_form(form)
    got = call(op, shaped(X, (X.shape[2],)), None if Y is None else shaped(Y, (Y.shape[2],)), n=n, seeds=shaped(seeds, ()), e=e)
    ran = bfs.last_form()
    bfs.set_form(None)
    return got, ran


# ---- every bit, both forms, every boundary -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", OPS)
def test_bit_exact_against_the_oracle(op, kind, orcb, OTPB):
    seen = {}
    with np.errstate(all="ignore"):
        for n, B, nx, ny, e, forms in bit_exact_cases(op):
            X, Y, want = expected(orcb, OTPB, op, kind, n, B, nx, ny, e)
            if kind in FINITE:
                assert np.isfinite(want).all()  # nothing is masked below
            seeds = host_seeds(orcb, op, X) if op in ("exp", "log") else None
            ran_forms = set()
            for form in forms:
                got, ran = run(op, X, Y, n, form, seeds, e, batch=(3, 2) if B == 6 else None)
                what = f"{op} {kind} n={n} B={B} nx={nx} ny={ny} e={e} form={ran}"
                if op == "pow" and e == 0:
                    assert ran is None, what  # [{1, 0}, {0, 0}, ...]: no product ran
                else:
                    assert ran in ("A", "B"), what
                    if form == "B":
                        assert ran == "B", what
                assert_bits(got, want, what)
                ran_forms.add(ran)
                seen.setdefault(ran, []).append((n, B))
            if op == "pow" and e == 0:
                continue
            if forms == ("A", "B"):
                if n <= FORM_A_MAX_PLAIN[op]:
                    assert ran_forms == {"A", "B"}, (n, B, ran_forms)  # short rows fit form A: both forms were compared
                if n > FORM_A_MAX[op]:
                    assert ran_forms == {"B"}, (n, B, ran_forms)
            elif B >= 256 and op not in ("exp", "log"):
                assert ran_forms == {"A"}, (n, B, ran_forms)  # n = 9 from 256 items on: the automatic choice is form A
    assert seen.get("A") and seen.get("B")


def test_dispatch_by_batch_size():
    """the thresholds are the interval family's: short rows take form A from 256 items on, form B below; exp / log whenever they fit"""
    from genfer_amd import bigfloat_series as bfs

    for n, B, want in [(9, 256, "A"), (9, 255, "B"), (31, 256, "A"), (40, 300, "B")]:
        x, y = dev(data("near", B, n, 5)), dev(data("near", B, n, 6))
        for f in (bfs.mul, bfs.div):
            f(x, y)
            assert bfs.last_form() == want, (n, B)
    bfs.compose(dev(data("near", 300, 21, 5)), dev(data("near", 300, 21, 6)))
    assert bfs.last_form() == "A"
    bfs.compose(dev(data("near", 300, 26, 5)), dev(data("near", 300, 26, 6)))
    assert bfs.last_form() == "B"
    bfs.exp(dev(data("near", 3, 24, 5)))
    assert bfs.last_form() == "A"
    bfs.log(dev(data("near", 3, 64, 5)))
    assert bfs.last_form() == "B"


@pytest.mark.parametrize("form", ["A", "B"])
def test_the_addition_onto_the_zeroed_result_is_performed(form, orcb):
    """mul_rec adds every finished sum onto a zero; for BigFloat that drops a sum whose exponent fell to -1024 or below by cancellation.
    The crafted operands (tests/test_bigfloat_series_cpu.py) have such a sum at coefficient 1, in mul and inside compose's second step."""
    x, y, n = crafted()["mul"]
    X, Y = np.repeat(x[:, None], 5, axis=1), np.repeat(y[:, None], 5, axis=1)
    want = want_mul(orcb, X, Y, n)
    assert want[:, 0].tolist() == [[1.125, 0.0], [-1021.0, 0.0]]
    got, ran = run("mul", X, Y, n, form)
    assert ran == form
    assert_bits(got, want, f"mul form {form}")
    f, g, n = crafted()["compose"]
    F, G = np.repeat(f[:, None], 5, axis=1), np.repeat(g[:, None], 5, axis=1)
    want = want_compose(orcb, F, G, n)
    assert want[:, 0, 1].tolist() == [0.0, 0.0]
    got, ran = run("compose", F, G, n, form)
    assert ran == form
    assert_bits(got, want, f"compose form {form}")
    # pow's products are mul's: x^2 * 1 through the same operands' square
    got, ran = run("pow", X, None, 3, form, e=2)
    assert_bits(got, want_pow(orcb, X, 2, 3), f"pow form {form}")


# ---- layouts -------------------------------------------------------------------------------------------------------------------------

VIEW_N, VIEW_BATCH = 12, (3, 2)


def view_case(op, orcb, OTPB, kind="wide"):
    B = int(np.prod(VIEW_BATCH))
    x, y, want = expected(orcb, OTPB, op, kind, VIEW_N, B, VIEW_N, VIEW_N, 3)
    sd = host_seeds(orcb, op, x) if op in ("exp", "log") else None
    return x, y, want, sd


@pytest.mark.parametrize("op", OPS)
def test_views(op, orcb, OTPB):
    from genfer_amd import bigfloat_series as bfs

    n, batch = VIEW_N, VIEW_BATCH
    B, nb = int(np.prod(batch)), len(batch)
    x, y, want, sd = view_case(op, orcb, OTPB)
    full = (2,) + batch + (n,)
    want = want.reshape(full)
    X = dev(x).reshape(full)
    Y = dev(y).reshape(full) if y is not None else None
    S = dev(sd).reshape((2,) + batch) if sd is not None else None
    assert_bits(call(op, X, Y, seeds=S), want, "contiguous")
    # planes and rows sliced out of a wider, longer buffer: a plane stride that is not items * n
    wide = torch.zeros((3,) + batch + (n + 9,), dtype=torch.float64, device=DEV)
    wide[::2][..., 4:4 + n] = X
    xs = wide[::2][..., 4:4 + n]
    assert not xs.is_contiguous() and xs.stride(0) == 2 * B * (n + 9)
    assert_bits(call(op, xs, Y, seeds=S), want, "planes out of a wider buffer")
    # the planes interleaved per item ([B..., 2, n] seen as [2, B..., n]): the plane stride is below the batch strides
    inter = torch.stack([X[0], X[1]], dim=nb).movedim(nb, 0)
    assert inter.stride(0) == n and not inter.is_contiguous()
    assert_bits(call(op, inter, Y, seeds=S), want, "interleaved planes")
    # a transposed batch, as an operand and as out
    perm = (0, 2, 1, 3)
    xp = X.permute(*perm).contiguous().permute(*perm)
    assert not xp.is_contiguous() and xp.stride(-1) == 1
    assert_bits(call(op, xp, Y, seeds=S), want, "transposed batch")
    po = torch.empty(tuple(full[i] for i in perm), dtype=torch.float64, device=DEV).permute(*perm)
    call(op, X, Y, out=po, seeds=S)
    assert_bits(po, want, "transposed out")
    # a sliced out, its planes 2 apart in a wider buffer, with guard words around every row and a whole guard plane between
    big = torch.full((3,) + batch + (n + 5,), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
    out = big[::2][..., 2:2 + n]
    assert call(op, xs, Y, out=out, seeds=S) is out
    assert_bits(out, want, "sliced out")
    g = big.view(torch.int64)
    assert bool((g[..., :2] == GUARD).all()) and bool((g[..., 2 + n:] == GUARD).all()) and bool((g[1] == GUARD).all())
    # out as an operand's same view, both forms
    for form in ("A", "B"):
        bfs.set_form(form)
        xi = X.clone()
        assert call(op, xi, Y, out=xi, seeds=S) is xi
        assert_bits(xi, want, f"{op} in place on x, form {form}")
        if Y is not None:
            yi = Y.clone()
            call(op, X, yi, out=yi)
            assert_bits(yi, want, f"{op} in place on y, form {form}")
    bfs.set_form(None)


@pytest.mark.parametrize("op", ["mul", "div", "compose"])
def test_one_series_against_every_item(op, orcb, OTPB):
    """batch stride 0: one series (with its two planes) against the batch, on either side"""
    n, B = 12, 7
    x, y = operands(op, "wide", n, B, n, n)
    y0 = np.repeat(y[:, :1], B, axis=1)
    one = dev(y[:, 0])  # [2, n]
    wx = expected_for(op, x, y0, n, orcb, OTPB)
    assert_bits(call(op, dev(x), one[:, None, :].expand(2, B, n)), wx, "expanded y")
    assert_bits(call(op, dev(x), one), wx, "broadcast [2, n] y")
    wy = expected_for(op, y0, x, n, orcb, OTPB)
    assert_bits(call(op, one, dev(x)), wy, "broadcast [2, n] x")


def expected_for(op, X, Y, n, orcb, OTPB):
    if op == "mul":
        return want_mul(orcb, X, Y, n)
    if op == "compose":
        return want_compose(orcb, X, Y, n)
    return want_handle(orcb, OTPB, op, X, Y, n)


def test_planes_from_two_allocations(orcb):
    """the factor plane and the exponent plane of every tensor in allocations of their own, joined by a large plane stride: through the
    C entry point, whose stride arrays start with the factor -> exponent plane stride"""
    import genfer_amd
    from genfer_amd import bigfloat_series as bfs

    n, B = 16, 5
    x, y = data("wide", B, n, 61), data("wide", B, n, 62)
    want = want_mul(orcb, x, y, n)
    bfs.last_form()  # declares the entry points
    L = genfer_amd.lib()
    # six allocations of 4 MiB, sorted by address: x's planes, y's planes, the result's planes -- each tensor's span then holds no other's
    blocks = sorted((torch.zeros(1 << 19, dtype=torch.float64, device=DEV) for _ in range(6)), key=lambda t: t.data_ptr())
    assert len({t.data_ptr() for t in blocks}) == 6
    for k, src in enumerate((x[0], x[1], y[0], y[1])):
        blocks[k][:B * n] = dev(src).reshape(-1)
    guard = torch.full((1 << 19,), GUARD, dtype=torch.int64, device=DEV)
    for k in (4, 5):
        blocks[k].view(torch.int64).copy_(guard)
    stride = lambda a, b: (b.data_ptr() - a.data_ptr()) // 8  # noqa: E731
    arrs = [(C.c_int64 * 2)(stride(blocks[2 * k], blocks[2 * k + 1]), n) for k in range(3)]
    assert all(a[0] >= 1 << 19 for a in arrs)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    shape = (C.c_size_t * 1)(B)
    torch.cuda.synchronize()
    rc = L.gftb_series_mul(vp(blocks[0]), arrs[0], n, vp(blocks[2]), arrs[1], n, vp(blocks[4]), arrs[2], n, shape, 1,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.gft_last_error()
    torch.cuda.synchronize()
    got = torch.stack([blocks[4][:B * n], blocks[5][:B * n]]).reshape(2, B, n)
    assert_bits(got, want, "planes from two allocations")
    for k in (4, 5):
        assert bool((blocks[k].view(torch.int64)[B * n:] == GUARD).all())


def test_empty_batch_is_a_no_op():
    from genfer_amd import bigfloat_series as bfs

    z = bfs.mul(torch.zeros((2, 0, 8), dtype=torch.float64, device=DEV), torch.zeros((2, 0, 8), dtype=torch.float64, device=DEV))
    assert z.shape == (2, 0, 8)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------


def test_refusals_name_the_cause(orcb):
    import genfer_amd
    from genfer_amd import bigfloat_series as bfs
    from genfer_amd.taylor import TaylorError

    x, y = dev(data("near", 6, 16, 1)), dev(data("near", 6, 16, 2))

    def after():  # no stale HIP error: torch's next call succeeds
        assert float((x[0].abs() + 1.0).sum().item()) > 0

    with pytest.raises(TaylorError, match="out: .*plane stride 0"):  # a plane stride of 0 is judged by the Python side, on out too
        bfs.mul(x, y, out=torch.empty((6, 16), dtype=torch.float64, device=DEV).expand(2, 6, 16))
    after()
    with pytest.raises(TaylorError, match="x: .*plane stride 0"):
        bfs.mul(x[0].expand(2, 6, 16), y)
    after()
    with pytest.raises(TaylorError, match="zero stride"):
        bfs.mul(x, y, out=torch.empty((2, 1, 16), dtype=torch.float64, device=DEV).expand(2, 6, 16))
    after()
    # overlapping result planes: the exponent plane starts inside the factor plane
    flat = torch.empty(2 * 6 * 16, dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="overlap"):
        bfs.mul(x, y, out=flat.as_strided((2, 6, 16), (40, 16, 1)))
    after()
    # partial overlap across planes: the result's factor plane is x's exponent plane
    buf = torch.rand((3, 6, 16), dtype=torch.float64, device=DEV)
    for f in (bfs.mul, bfs.div, bfs.compose):
        with pytest.raises(TaylorError, match="partially overlaps (x|f)"):
            f(buf[0:2], y, out=buf[1:3])
        after()
        with pytest.raises(TaylorError, match="partially overlaps (y|g)"):
            f(y, buf[0:2], out=buf[1:3])
        after()
    for f in (bfs.exp, bfs.log, lambda t, out: bfs.pow(t, 3, out=out)):
        with pytest.raises(TaylorError, match="partially overlaps x"):
            f(buf[0:2], out=buf[1:3])
        after()
    # ... and the same storage with another plane stride is not "the same view"
    buf4 = torch.rand((4, 6, 16), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps x"):
        bfs.mul(buf4[0::2], y, out=buf4[0::3])
    after()
    with pytest.raises(TaylorError, match="2048"):
        bfs.mul(x, y, n=2049)
    after()
    # through the C entry points: the plane stride 0 of an operand and of the seeds, the library's own limit, n == 0, nx > n
    bfs.last_form()  # declares the entry points
    L = genfer_amd.lib()
    one = (C.c_size_t * 1)(6)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    z = torch.empty_like(x)
    point, planes = (C.c_int64 * 2)(0, 16), (C.c_int64 * 2)(96, 16)
    assert L.gftb_series_mul(vp(x), point, 16, vp(y), None, 16, vp(z), None, 16, one, 1, None) == -1
    assert L.gft_last_error().decode().startswith("bigfloat series_mul: zero plane stride on x")
    assert L.gftb_series_compose(vp(x), None, 16, vp(y), point, 16, vp(z), None, 16, one, 1, None) == -1
    assert L.gft_last_error().decode().startswith("bigfloat series_compose: zero plane stride on g")
    assert L.gftb_series_exp(vp(x), planes, 16, vp(y), (C.c_int64 * 2)(0, 1), vp(z), None, 16, one, 1, None) == -1
    assert L.gft_last_error().decode().startswith("bigfloat series_exp: zero plane stride on the seeds")
    for fn in (L.gftb_series_mul, L.gftb_series_div, L.gftb_series_compose):
        assert fn(vp(x), None, 16, vp(y), None, 16, vp(z), None, 2049, one, 1, None) == -1
        assert "2048" in L.gft_last_error().decode() and L.gft_last_error().decode().startswith("bigfloat series_")
    assert L.gftb_series_log(vp(x), None, 16, None, None, vp(z), None, 2049, one, 1, None) == -1
    assert "2048" in L.gft_last_error().decode()
    assert L.gftb_series_pow(vp(x), None, 16, 3, vp(z), None, 2049, one, 1, None) == -1
    assert "2048" in L.gft_last_error().decode()
    assert L.gftb_series_mul(vp(x), None, 16, vp(y), None, 16, vp(z), None, 0, one, 1, None) == -1
    assert "n == 0" in L.gft_last_error().decode()
    assert L.gftb_series_mul(vp(x), None, 16, vp(y), None, 4, vp(z), None, 8, one, 1, None) == -1
    assert "nx = 16 > n = 8" in L.gft_last_error().decode()
    after()
    # NULL strides: C-contiguous rows, the planes back to back
    assert L.gftb_series_mul(vp(x), None, 16, vp(y), None, 16, vp(z), None, 16, one, 1, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(z), bits(bfs.mul(x, y)))
    assert_bits(z, want_mul(orcb, x.cpu().numpy(), y.cpu().numpy(), 16), "after the refusals")


# ---- device seeds --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,B", [(16, 300), (39, 65), (100, 3)])
def test_device_seeds(n, B, orcb, OTPB):
    """seed=None: coefficient 0 of exp and log, decoded, within REL_TOL of the oracle's, on inputs whose seeds stay inside the f64 range
    (|x0| < 2^4 for exp, any exponent of +-20 for log); log's coefficients k >= 1 do not depend on the seed: bit for bit; exp's result
    is, bit for bit, that of a second call given the first call's coefficient 0 as its seed"""
    from genfer_amd import bigfloat_series as bfs

    for op in ("exp", "log"):
        X = data("near", B, n, 31 * n + B, head=(-6, 3) if op == "exp" else (-20, 20))
        want = want_handle(orcb, OTPB, op, X, None, n)
        got = run(op, X, None, n)[0]
        g0, w0 = bfs.decode(got[..., 0]).cpu().numpy(), bfs.decode(dev(want[..., 0])).cpu().numpy()
        assert np.isfinite(w0).all() and (w0 != 0).all()
        print(f"{op} n={n} B={B}: device seed off by at most {np.max(np.abs(g0 - w0) / np.abs(w0)):.3e} (relative)")
        assert np.all(np.abs(g0 - w0) <= REL_TOL * np.abs(w0)), (op, n, B, np.max(np.abs(g0 - w0) / np.abs(w0)))
        if op == "log":
            assert_bits(got[..., 1:], want[..., 1:], f"log n={n} B={B} device seed, k >= 1")
        else:
            again = bfs.exp(dev(X), n=n, seed=got[..., 0].contiguous())
            assert torch.equal(bits(again), bits(got)), f"exp n={n} B={B}: the device seed as seed="


# ---- round trip ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,B", [(24, 300), (40, 65), (200, 5)])
def test_round_trip_against_the_f64_series(n, B):
    """decode(mul(encode(x), encode(y))) equals series.mul(x, y) within REL_TOL on moderate positive data, where no BigFloat rule (drop,
    cut-off) can fire: every term and every sum lies within 2^+-40 of 1"""
    from conftest import splitmix64_uniform
    from genfer_amd import bigfloat_series as bfs
    from genfer_amd import series

    x = dev(0.5 + splitmix64_uniform(3 * n + B, B * n).reshape(B, n))
    y = dev(0.5 + splitmix64_uniform(5 * n + B, B * n).reshape(B, n))
    got = bfs.decode(bfs.mul(bfs.encode(x), bfs.encode(y)))
    want = series.mul(x, y)
    rel = ((got - want).abs() / want.abs()).max().item()
    print(f"n={n} B={B}: round trip off by at most {rel:.3e} (relative)")
    assert rel <= REL_TOL


# ---- streams -------------------------------------------------------------------------------------------------------------------------


def test_ordered_on_a_non_default_current_stream(orcb):
    """the call is ordered on torch's current stream: behind the copy that fills its operand there, in front of its consumer and of the
    operand's reuse, with no host synchronisation in between"""
    from genfer_amd import bigfloat_series as bfs

    B, n = 256, 24
    x, y = data("wide", B, n, 41), data("wide", B, n, 42)
    want = want_mul(orcb, x, y, n)
    X, Y = dev(x), dev(y)
    src = torch.zeros((2, B, n), dtype=torch.float64, device=DEV)
    bfs.mul(src, Y)  # warm the kernel
    filler = torch.ones(1 << 24, dtype=torch.float64, device=DEV)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(40):
            filler.mul_(1.0000001)  # work queued on this stream in front of the operand's copy
        src.copy_(X)  # the operand is produced on this stream
        z = bfs.mul(src, Y)
        dec = bfs.decode(z)  # consumed right after, no host synchronisation in between
        src.zero_()  # the operand is reused right after
    s.synchronize()
    assert_bits(z, want, "mul on a side stream")
    assert torch.equal(bits(dec), bits(bfs.decode(dev(want)))), "the consumer on the side stream"
