"""Batched interval series on device tensors (genfer_amd.interval_series, gfti_series_*) on the MI355X.

Every bound of every coefficient of every item carries the oracle's bits, in both forms of the kernels and on both sides of
every dispatch boundary, on positive, mixed-sign and special-valued rows; views with every kind of plane stride, broadcasting,
in-place results, guard words, refusals, device seeds, enclosure of the f64 series and the stream contract.  The data, the cases'
expected values (the shim's product, the oracle's handle operators, the chains) come from tests/test_interval_series_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import REL_TOL
from test_interval_series_cpu import (KINDS, data, host_seeds, shim, want_compose, want_handle, want_mul, want_pow)  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 0x5A5A5A5A5A5A5A5A
OPS = ("mul", "div", "exp", "log", "compose", "pow")


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield
    genfer_amd.interval_series.set_form(None)


@pytest.fixture(autouse=True)
def _auto_form():
    from genfer_amd import interval_series as ivs

    ivs.set_form(None)
    yield
    ivs.set_form(None)


def assert_bits(got, want, what):
    """every bit of every bound; where the oracle's value is NaN, a NaN (tests/test_series_batch_gpu.py's rule)"""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    want = np.ascontiguousarray(want)
    got = np.ascontiguousarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    ok = np.where(nan, np.isnan(got), got.view(np.int64) == want.view(np.int64))
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {(~ok).sum()} bounds differ, first at {i}: got {got[i]!r} want {want[i]!r}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# both sides of every boundary of the dispatch: form A's waves per workgroup change at n = 9 | 10 and 19 | 20 (compose: 13 | 14 is
# inside 10 .. 19), compose leaves form A at 25 | 26, the others at 39 | 40; 64 | 65 is the staging width; long rows beyond
ORDERS = [1, 2, 3, 9, 10, 19, 20, 25, 26, 39, 40, 64, 65, 257, 1024, 2048]
BATCHES = [1, 3, 64, 65, 1000]
POW_E = [0, 1, 2, 5, 13]
# The oracle side of this file stays within that of the two f64 files (tests/test_series_batch_gpu.py, tests/test_series_compose_gpu.py).
# tests/test_interval_series_cpu.py::test_oracle_side_stays_within_the_f64_files measures both on the host it runs on, one after the
# other on one thread, and asserts the bound.  On the development host (its timings move by a third between runs; three runs gave the
# interval side 0.59, 0.76 and 0.80 of the f64 side) the last run took: the bit-exact loops of the f64 files 14.3 s (mul / div / exp / log
# 11.3, compose 1.8, pow 1.2); every expected value of this file 8.4 s (bit-exact mul 0.8, div 2.0, exp 1.2, log 1.2, compose 1.5, pow
# 1.0; the other tests 0.7).  The interval oracle costs 0.08 - 0.31 s per 1e7 of B * n^2 (mul 0.08 - 0.15, div 0.19 - 0.31, exp / log
# 0.14 - 0.16), a handle operator or a product of a chain costs 25 - 45 us of Python per item whatever n, and every case runs on three
# data sets, so:
# - B * n^2 <= 2.5e6 per case, and one row (B = 1) at every order: B = 64 and 65 run up to n = 65, B = 3 up to n = 257, n = 1024 and
#   2048 at B = 1;
# - B = 1000 runs on BIG_BATCH_ORDERS, the two sides of the form-A boundaries (what 256 items and more change is the choice of form A);
# - LONG_ROWS adds (2048, 3) with compact operands for mul, div and compose: the long-row kernels of form B (k_div_1d_batch among them)
#   with more than one item;
# - compose: B * nf * n^2 within the same budget (at least nf = 2) and B * nf <= CHAIN_STEPS products per case;
# - pow: on the orders up to 257; the full exponent list on B = 1 and 65, e = 3 at B = 1000 on four orders (its products are mul's).
CPU_BUDGET = 2.5e6
CHAIN_STEPS = 400
LONG_ROWS = [(2048, 3)]
BIG_BATCH_ORDERS = [9, 10, 19, 20, 25, 26, 39, 40]  # the two sides of the form-A boundaries, where 256 items and more choose form A
# the shapes of the other tests that ask the oracle (their share of the time above)
VIEW_SHAPES = [(12, (5, 70)), (24, (3, 4, 6)), (130, (2, 5)), (20, (7,))]
POINT_SHAPES = [(12, 300), (24, 7), (130, 5)]
SEED_SHAPES = [(16, 1000), (39, 65), (100, 3), (300, 64)]
STREAM_SHAPE = (512, 24)


def cases(op=None):
    for n in ORDERS:
        for B in BATCHES:
            if B > 1 and B * n * n > CPU_BUDGET and not (op in ("mul", "div", "compose") and (n, B) in LONG_ROWS):
                continue
            if B == 1000 and n not in BIG_BATCH_ORDERS:
                continue
            yield n, B


def lengths(op, n, B):
    """(nx, ny): dense, and compact operands (nx < n, ny < n, nx = 1) on some of the batches; the divisor of div and the operand of
    exp / log keep at least two coefficients, so the oracle's operators take their general path"""
    out = [(n, n)]
    if n >= 3 and B in (3, 65):
        out += [(n // 2, n - 1), (1, max(2, n // 3) if op == "mul" else n)]
    if (n, B) in LONG_ROWS:
        out = [(n // 2, 65)]  # (the dense pair of a long row ran at B = 1)
    if op in ("exp", "log"):
        out = sorted({(max(nx, 2), max(nx, 2)) for nx, _ in out if n >= 2})
    return out


def compose_lengths(n, B):
    """(nf, ng) within the budget: dense where it fits, else the longest f that fits against a dense g; the compact corners"""
    top = max(2, min(int(CPU_BUDGET // (B * n * n)), CHAIN_STEPS // B))
    out = [(min(n, top), n)]
    if B == 65 or (B == 3 and n > 65):
        for nf, ng in [(1, n), (2, n), (min(n, top), 1), (min(n, top), 2), (min(n // 2 + 1, top), n // 2 + 2)]:
            if 1 <= nf <= n and 1 <= ng <= n and (nf, ng) not in out:
                out.append((nf, ng))
    if (n, B) in LONG_ROWS:
        out = [(2, n), (2, n // 2 + 2)]
    return out


def operands(kind, n, B, nx, ny):
    return data(kind, B, nx, 1000 * n + B + 31 * nx), data(kind, B, ny, 2000 * n + B + 7 + 17 * ny)


def expected(op, kind, n, B, nx, ny, OTPI, oracle_lib, shim, e=None):
    """the operands of a case and the oracle's result"""
    X, Y = operands(kind, n, B, nx, ny)
    if op == "mul":
        return X, Y, want_mul(shim, X, Y, n)
    if op == "compose":
        return X, Y, want_compose(shim, oracle_lib, X, Y, n)
    if op == "pow":
        return X, None, want_pow(shim, X, e, n)
    return X, Y, want_handle(OTPI, op, X, Y, n)


def bit_exact_cases(op):
    """(n, B, nx, ny, e) of the bit-exact test of `op`"""
    for n, B in cases(op):
        if op == "compose":
            for nf, ng in compose_lengths(n, B):
                yield n, B, nf, ng, None
        elif op == "pow":
            if n <= 257 and B in (1, 65, 1000) and not (B == 1000 and n not in (19, 20, 39, 40)):
                for nx in sorted({n, max(1, n // 3)}) if B < 1000 else (n,):
                    for e in (POW_E if nx == n and B < 1000 else (3 if B == 1000 else 5,)):
                        if B * n * n * max(1, e.bit_length()) <= 4 * CPU_BUDGET:
                            yield n, B, nx, 1, e
        else:
            if op in ("div", "exp", "log") and n < 2:
                continue  # a one-coefficient divisor / operand is the operators' shortcut, not the recurrence
            for nx, ny in lengths(op, n, B):
                yield n, B, nx, ny, None


def oracle_side_seconds(OTPI, oracle_lib, shim):
    """the CPU seconds of every expected value this file asks the oracle for, per test (the CPU test named at CPU_BUDGET calls this)"""
    import time

    took = {}
    with np.errstate(all="ignore"):
        for op in OPS:
            t0 = time.time()
            for kind in KINDS:
                for n, B, nx, ny, e in bit_exact_cases(op):
                    X = expected(op, kind, n, B, nx, ny, OTPI, oracle_lib, shim, e)[0]
                    if op in ("exp", "log"):
                        host_seeds(oracle_lib, op, X)
            took[op] = time.time() - t0
        t0 = time.time()
        for op in OPS:
            for n, batch in VIEW_SHAPES:
                X = expected(op, "mixed", n, int(np.prod(batch)), n, n, OTPI, oracle_lib, shim, 3)[0]
                if op in ("exp", "log"):
                    host_seeds(oracle_lib, op, X)
            for n, B in POINT_SHAPES:
                if op in ("mul", "div", "compose"):
                    x, y = operands("pos", n, B, n, n)
                    y0 = np.repeat(y[:, :1], B, axis=1)
                    expected_for(op, x, y0, n, OTPI, oracle_lib, shim)
                    expected_for(op, y0, x, n, OTPI, oracle_lib, shim)
        for n, B in SEED_SHAPES:
            for op in ("exp", "log"):
                want_handle(OTPI, op, data("pos", B, n, 31 * n + B), None, n)
        B, n = STREAM_SHAPE
        for _ in range(2):
            want_mul(shim, data("mixed", B, n, 41), data("mixed", B, n, 42), n)
        want_mul(shim, data("pos", 6, 16, 1), data("pos", 6, 16, 2), 16)
        took["others"] = time.time() - t0
    return took


def run(op, X, Y, n, form=None, seeds=None, e=None):
    """X, Y: numpy [2, B, nx] / [2, B, ny]; the batched call in the asked form, and the form that ran"""
    from genfer_amd import interval_series as ivs

    ivs.set_form(form)
    if op in ("mul", "div", "compose"):
        got = getattr(ivs, op)(dev(X), dev(Y), n=n)
    elif op == "pow":
        got = ivs.pow(dev(X), e, n=n)
    else:
        got = getattr(ivs, op)(dev(X), n=n, seed=None if seeds is None else dev(seeds))
    ran = ivs.last_form()
    ivs.set_form(None)
    return got, ran


FORM_A_MAX = {"mul": 39, "div": 39, "exp": 39, "log": 39, "compose": 25, "pow": 39}  # gft_series.hip: 2 (3) arrays of two planes in 80 KB
FORM_A_MAX_PLAIN = {"mul": 31, "div": 31, "exp": 31, "log": 31, "compose": 21, "pow": 31}  # where the runtime grants 64 KB only


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", OPS)
def test_bit_exact_against_the_oracle(op, kind, OTPI, oracle_lib, shim):
    seen = {}
    with np.errstate(all="ignore"):
        for n, B, nx, ny, e in bit_exact_cases(op):
            X, Y, want = expected(op, kind, n, B, nx, ny, OTPI, oracle_lib, shim, e)
            seeds = host_seeds(oracle_lib, op, X) if op in ("exp", "log") else None
            forms = set()
            for form in (None, "A", "B"):
                got, ran = run(op, X, Y, n, form, seeds, e)
                what = f"{op} {kind} n={n} B={B} nx={nx} ny={ny} e={e} form={ran}"
                if op == "pow" and e == 0:
                    assert ran is None, what  # [1, 0, ...]: no product ran
                else:
                    assert ran in ("A", "B"), what
                    if form == "B":
                        assert ran == "B", what
                assert_bits(got, want, what)
                forms.add(ran)
                seen.setdefault(ran, []).append((n, B))
            if op == "pow" and e == 0:
                continue
            if n <= FORM_A_MAX_PLAIN[op]:
                assert forms == {"A", "B"}, (n, B, forms)  # short rows fit form A: both forms were compared
            if n > FORM_A_MAX[op]:
                assert forms == {"B"}, (n, B, forms)
    assert seen.get("A") and seen.get("B")


def test_dispatch_by_batch_size():
    """the thresholds: short rows take form A from 256 items on, form B below; rows beyond the interval budget always form B.  The
    orders asked to take form A fit it with the 64 KB the runtime always grants too (n <= 31, compose n <= 21)."""
    from genfer_amd import interval_series as ivs

    for n, B, want in [(9, 1000, "A"), (16, 65, "B"), (31, 256, "A"), (31, 255, "B"), (40, 1000, "B"), (19, 3, "B")]:
        x, y = dev(data("pos", B, n, 5)), dev(data("pos", B, n, 6))
        for f in (ivs.mul, ivs.div):
            f(x, y)
            assert ivs.last_form() == want, (n, B)
    for n, B, want in [(21, 300, "A"), (26, 300, "B"), (21, 100, "B")]:
        ivs.compose(dev(data("pos", B, n, 5)), dev(data("pos", B, n, 6)))
        assert ivs.last_form() == want, (n, B)
    ivs.exp(dev(data("pos", 3, 24, 5)))
    assert ivs.last_form() == "A"
    ivs.log(dev(data("pos", 3, 64, 5)))
    assert ivs.last_form() == "B"


# ---- views -----------------------------------------------------------------------------------------------------------------------


def call(op, x, y, n=None, out=None, seeds=None):
    from genfer_amd import interval_series as ivs

    if op in ("mul", "div", "compose"):
        return getattr(ivs, op)(x, y, n=n, out=out)
    if op == "pow":
        return ivs.pow(x, 3, n=n, out=out)
    return getattr(ivs, op)(x, n=n, seed=seeds, out=out)


@pytest.mark.parametrize("n,batch", VIEW_SHAPES)
@pytest.mark.parametrize("op", OPS)
def test_views(op, n, batch, OTPI, oracle_lib, shim):
    from genfer_amd import interval_series as ivs

    B, nb = int(np.prod(batch)), len(batch)
    x, y, want = expected(op, "mixed", n, B, n, n, OTPI, oracle_lib, shim, 3)
    full = (2,) + batch + (n,)
    want = want.reshape(full)
    X = dev(x).reshape(full)
    Y = dev(y).reshape(full) if y is not None else None
    sd = dev(host_seeds(oracle_lib, op, x)).reshape((2,) + batch) if op in ("exp", "log") else None
    # a plane stride that is not items * n, and a sliced series axis: planes cut out of a wider, longer buffer
    wide = torch.zeros((3,) + batch + (n + 9,), dtype=torch.float64, device=DEV)
    wide[::2][..., 4:4 + n] = X
    xs = wide[::2][..., 4:4 + n]
    assert not xs.is_contiguous() and xs.stride(0) == 2 * B * (n + 9)
    assert_bits(call(op, xs, Y, seeds=sd), want, "planes out of a wider buffer")
    # the planes interleaved per item ([B..., 2, n] seen as [2, B..., n]): the plane stride is below the batch strides
    inter = torch.stack([X[0], X[1]], dim=nb).movedim(nb, 0)
    assert inter.stride(0) == n and not inter.is_contiguous()
    assert_bits(call(op, inter, Y, seeds=sd), want, "interleaved planes")
    # batch axes permuted (a non-contiguous batch)
    if nb >= 2:
        perm = (0,) + tuple(reversed(range(1, nb + 1))) + (nb + 1,)
        xp = X.permute(*perm).contiguous().permute(*perm)
        assert not xp.is_contiguous() and xp.stride(-1) == 1
        assert_bits(call(op, xp, Y, seeds=sd), want, "permuted batch")
        po = torch.empty(tuple(full[i] for i in perm), dtype=torch.float64, device=DEV).permute(*perm)
        call(op, X, Y, out=po, seeds=sd)
        assert_bits(po, want, "permuted out")
    # a sliced out, its planes 2 apart in a wider buffer, with guards around every row and a whole guard plane between
    big = torch.full((3,) + batch + (n + 5,), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
    out = big[::2][..., 2:2 + n]
    assert call(op, xs, Y, out=out, seeds=sd) is out
    assert_bits(out, want, "sliced out")
    g = big.view(torch.int64)
    assert bool((g[..., :2] == GUARD).all()) and bool((g[..., 2 + n:] == GUARD).all()) and bool((g[1] == GUARD).all())
    # in place, both forms
    for form in ("A", "B"):
        ivs.set_form(form)
        xi = X.clone()
        assert call(op, xi, Y, out=xi, seeds=sd) is xi
        assert_bits(xi, want, f"{op} in place on x, form {form}")
        if op in ("mul", "div", "compose"):
            yi = Y.clone()
            call(op, X, yi, out=yi)
            assert_bits(yi, want, f"{op} in place on y, form {form}")
    ivs.set_form(None)


@pytest.mark.parametrize("n,B", POINT_SHAPES)
@pytest.mark.parametrize("op", OPS)
def test_point_intervals_and_one_series_against_a_batch(op, n, B, OTPI, oracle_lib, shim):
    """plane stride 0: x.expand(2, ...) equals the same call on materialised planes; batch stride 0: one series against a batch"""
    x, y = operands("pos", n, B, n, n)
    P = dev(x[0])  # [B, n] point values
    Pe = P.expand(2, B, n)
    assert Pe.stride(0) == 0
    Y = dev(y) if op in ("mul", "div", "compose") else None
    sd = None
    if op in ("exp", "log"):
        s0 = getattr(torch, op)(P[:, 0])
        sd = s0.expand(2, B)  # point seeds, stride 0 on their plane axis as well
    got = call(op, Pe, Y, seeds=sd)
    assert torch.equal(bits(got), bits(call(op, Pe.contiguous(), Y, seeds=None if sd is None else sd.contiguous()))), "plane stride 0"
    if Y is not None:
        Ye = dev(y[0]).expand(2, B, n)
        assert torch.equal(bits(call(op, Pe, Ye)), bits(call(op, Pe.contiguous(), Ye.contiguous()))), "both operands points"
        # one series (with its two planes) against the batch, on either side
        y0 = np.repeat(y[:, :1], B, axis=1)
        one = dev(y[:, 0])  # [2, n]
        wx = expected_for(op, x, y0, n, OTPI, oracle_lib, shim)
        assert_bits(call(op, dev(x), one[:, None, :].expand(2, B, n)), wx, "expanded y")
        assert_bits(call(op, dev(x), one), wx, "broadcast [2, n] y")
        wy = expected_for(op, y0, x, n, OTPI, oracle_lib, shim)
        assert_bits(call(op, one, dev(x)), wy, "broadcast [2, n] x")


def expected_for(op, X, Y, n, OTPI, oracle_lib, shim):
    if op == "mul":
        return want_mul(shim, X, Y, n)
    if op == "compose":
        return want_compose(shim, oracle_lib, X, Y, n)
    return want_handle(OTPI, op, X, Y, n)


def test_empty_batch_is_a_no_op():
    from genfer_amd import interval_series as ivs

    z = ivs.mul(torch.zeros((2, 0, 8), dtype=torch.float64, device=DEV), torch.zeros((2, 0, 8), dtype=torch.float64, device=DEV))
    assert z.shape == (2, 0, 8)


# ---- refusals --------------------------------------------------------------------------------------------------------------------


def test_refusals_name_the_cause(shim):
    import genfer_amd
    from genfer_amd import interval_series as ivs
    from genfer_amd.taylor import TaylorError

    x, y = dev(data("pos", 6, 16, 1)), dev(data("pos", 6, 16, 2))

    def after():  # no stale HIP error: torch's next call succeeds
        assert float((x + 1.0).sum().item()) > 0

    with pytest.raises(TaylorError, match="zero plane stride"):
        ivs.mul(x, y, out=torch.empty((6, 16), dtype=torch.float64, device=DEV).expand(2, 6, 16))
    after()
    with pytest.raises(TaylorError, match="zero stride"):
        ivs.mul(x, y, out=torch.empty((2, 1, 16), dtype=torch.float64, device=DEV).expand(2, 6, 16))
    after()
    # overlapping result planes: the hi plane starts inside the lo plane
    flat = torch.empty(2 * 6 * 16, dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="overlap"):
        ivs.mul(x, y, out=flat.as_strided((2, 6, 16), (40, 16, 1)))
    after()
    # partial overlap across planes: the result's lo plane is x's hi plane
    buf = torch.rand((3, 6, 16), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps x"):
        ivs.mul(buf[0:2], y, out=buf[1:3])
    after()
    # ... and the same storage with another plane stride is not "the same view"
    buf4 = torch.rand((4, 6, 16), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps x"):
        ivs.mul(buf4[0::2], y, out=buf4[0::3])
    after()
    with pytest.raises(TaylorError, match="2048"):
        ivs.mul(x, y, n=2049)
    after()
    with pytest.raises(TaylorError, match="unit stride"):
        ivs.mul(torch.rand((2, 6, 32), dtype=torch.float64, device=DEV)[..., ::2], y)
    after()
    # through the C entry points: the library's own limit, n == 0, nx > n
    ivs.last_form()  # declares the entry points
    L = genfer_amd.lib()
    one = (C.c_size_t * 1)(6)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for fn in (L.gfti_series_mul, L.gfti_series_div, L.gfti_series_compose):
        assert fn(vp(x), None, 16, vp(y), None, 16, vp(y), None, 2049, one, 1, None) == -1
        assert "2048" in L.gft_last_error().decode()
    assert L.gfti_series_exp(vp(x), None, 16, None, None, vp(y), None, 2049, one, 1, None) == -1
    assert "2048" in L.gft_last_error().decode()
    assert L.gfti_series_pow(vp(x), None, 16, 3, vp(y), None, 2049, one, 1, None) == -1
    assert "2048" in L.gft_last_error().decode()
    assert L.gfti_series_mul(vp(x), None, 16, vp(y), None, 16, vp(y), None, 0, one, 1, None) == -1
    assert "n == 0" in L.gft_last_error().decode()
    assert L.gfti_series_mul(vp(x), None, 16, vp(y), None, 4, vp(y), None, 8, one, 1, None) == -1
    assert "nx = 16 > n = 8" in L.gft_last_error().decode()
    neg = (C.c_int64 * 2)(-96, 16)
    assert L.gfti_series_mul(vp(x), neg, 16, vp(y), None, 16, vp(torch.empty_like(x)), None, 16, one, 1, None) == -1
    assert "negative" in L.gft_last_error().decode()
    after()
    # NULL strides: C-contiguous rows, the planes back to back
    z = torch.empty_like(x)
    assert L.gfti_series_mul(vp(x), None, 16, vp(y), None, 16, vp(z), None, 16, one, 1, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(z), bits(ivs.mul(x, y)))
    assert_bits(z, want_mul(shim, x.cpu().numpy(), y.cpu().numpy(), 16), "after the refusals")


# ---- device seeds, enclosure -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,B", SEED_SHAPES)
def test_device_seeds(n, B, OTPI, oracle_lib):
    X = data("pos", B, n, 31 * n + B)
    for op in ("exp", "log"):
        want = want_handle(OTPI, op, X, None, n)
        got = run(op, X, None, n)[0].cpu().numpy()
        if op == "log":  # only coefficient 0 depends on the seed
            assert_bits(got[..., 1:], want[..., 1:], f"log n={n} B={B} device seed, k >= 1")
            got, want = got[..., :1], want[..., :1]
        assert np.all(np.abs(got - want) <= REL_TOL * np.abs(want)), (op, n, B, np.max(np.abs(got - want) / np.abs(want)))


@pytest.mark.parametrize("n,B", [(16, 300), (39, 65), (40, 65), (200, 5)])
@pytest.mark.parametrize("kind", ["pos", "mixed"])
def test_encloses_the_f64_series(n, B, kind):
    """lo = hi = x: every coefficient of every operation contains the f64 result on x (each interval operation rounds to nearest
    and steps one ulp outwards, so it contains the f64 operation on any points of its operands); NaN excepted"""
    from genfer_amd import interval_series as ivs
    from genfer_amd import series

    x, y = dev(data(kind, B, n, 3)[0]), dev(data(kind, B, n, 4)[0])
    xe, ye = x.expand(2, B, n), y.expand(2, B, n)
    pairs = [(series.mul(x, y), ivs.mul(xe, ye)), (series.div(x, y), ivs.div(xe, ye)), (series.exp(x), ivs.exp(xe)),
             (series.log(x), ivs.log(xe)), (series.compose(x[:, :6], y), ivs.compose(xe[..., :6], ye)), (series.pow(x, 5), ivs.pow(xe, 5))]
    for k, (p, iv) in enumerate(pairs):
        p, iv = p.cpu().numpy(), iv.cpu().numpy()
        ok = np.isnan(p) | np.isnan(iv[0]) | np.isnan(iv[1]) | ((iv[0] <= p) & (p <= iv[1]))
        assert ok.all(), (OPS[k], kind, n, B, int((~ok).sum()), tuple(np.argwhere(~ok)[0]))


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
def test_stream_ordered_without_host_stall(which, shim):
    from genfer_amd import interval_series as ivs

    B, n = STREAM_SHAPE
    x, y = data("mixed", B, n, 41), data("mixed", B, n, 42)
    want = want_mul(shim, x, y, n)
    X, Y = dev(x), dev(y)
    src = torch.zeros((2, B, n), dtype=torch.float64, device=DEV)
    ivs.mul(src, Y)  # warm the kernel
    cycles = _sleep_cycles_for_ms(100)
    s = torch.cuda.Stream() if which == "side_stream" else torch.cuda.default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        src.copy_(X)  # the operand is produced behind a long kernel on this stream
        z = ivs.mul(src, Y)
        twice = z * 2.0  # consumed right after, no host synchronisation in between
        src.zero_()  # the operand is reused right after
    s.synchronize()
    assert_bits(z, want, "mul on " + which)
    assert_bits(twice, want * 2.0, "consumer on " + which)


# ---- the handle API computes the same bits on the device ---------------------------------------------------------------------------


def test_agrees_with_the_handle_api(oracle_lib):
    import genfer_amd
    from genfer_amd import interval_series as ivs

    TPI = genfer_amd.IntervalTaylorPoly
    B, n = 6, 48
    x, y = data("mixed", B, n, 51), data("mixed", B, n, 52)
    X, Y = dev(x), dev(y)
    assert genfer_amd.lib().gft_set_conv_mode(3) == 0  # reference order
    try:
        zm, zd = ivs.mul(X, Y), ivs.div(X, Y)
        ze = ivs.exp(X, seed=dev(host_seeds(oracle_lib, "exp", x)))
        zl = ivs.log(X, seed=dev(host_seeds(oracle_lib, "log", x)))
        for b in range(B):
            p, q = TPI.from_torch(X[:, b]), TPI.from_torch(Y[:, b])
            assert torch.equal(bits(zm[:, b]), bits((p * q).to_torch())), b
            assert torch.equal(bits(zd[:, b]), bits((p / q).to_torch())), b
            assert torch.equal(bits(ze[:, b]), bits(p.exp().to_torch())), b
            assert torch.equal(bits(zl[:, b]), bits(p.log().to_torch())), b
    finally:
        assert genfer_amd.lib().gft_set_conv_mode(0) == 0
