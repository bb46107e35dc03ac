"""Batched compose and pow on device tensors (genfer_amd.series.compose / pow, gft_series_compose / gft_series_pow) on the MI355X.

Every coefficient of every item carries the bits of the definition: for dense data and ng >= 3 that is the oracle's own
subst_var / pow, everywhere else the chain of general products built from orc_mul_raw (test_series_compose_cpu.py shows the
two agree where both apply).  Both forms of the compose kernel, every side of the dispatch; views, broadcasting, in-place
results, refusals, the stream contract and the handle API."""
import ctypes as C

import numpy as np
import pytest

from test_series_compose_cpu import (POW_E, POW_SHAPES, compose_cases, compose_inputs, dense, oracle_compose, oracle_pow, want_compose,
                                     want_pow)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 0x5A5A5A5A5A5A5A5A
A_MAX_N, A_MAX_N_PLAIN = 53, 41  # the largest n compose takes in form A with 80 KB / 64 KB of LDS a workgroup (three arrays a wave)


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


def assert_bits(got, want, what):
    """every bit of every coefficient; where the expected value is NaN, a NaN"""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    ok = np.where(nan, np.isnan(got), got.view(np.int64) == want.view(np.int64))
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {(~ok).sum()} coefficients differ, first at {i}: got {got[i]!r} want {want[i]!r}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64)


def run_compose(f, g, n, form=None):
    from genfer_amd import series

    series.set_form(form)
    got = series.compose(dev(f), dev(g), n=n)
    ran = series.last_form()
    series.set_form(None)
    return got, ran


# ---- bit-exact against the oracle, per item, both forms, every side of the dispatch ---------------------------------------------


def test_compose_bit_exact_against_the_oracle(OTP, oracle_lib):
    seen, chosen = {}, set()
    for n, B, nf, ng in compose_cases():
        F, G = compose_inputs(n, B, nf, ng)
        # ng >= 3 and dense data: the oracle's subst_var is the expected value; else its operators shortcut and the chain is
        want = oracle_compose(OTP, F, G, n) if ng >= 3 else want_compose(oracle_lib, F, G, n)
        forms = set()
        for form in (None, "A", "B"):
            got, ran = run_compose(F, G, n, form)
            assert ran in ("A", "B")
            if form == "B":
                assert ran == "B"
            if form is None:
                chosen.add(ran)
            assert_bits(got, want, f"compose n={n} B={B} nf={nf} ng={ng} form={ran}")
            forms.add(ran)
            seen.setdefault(ran, []).append((n, B))
        if n <= A_MAX_N_PLAIN:
            assert forms == {"A", "B"}, (n, B, forms)  # short rows fit form A: both forms were compared
        if n > A_MAX_N:
            assert forms == {"B"}, (n, B, forms)
    assert seen.get("A") and seen.get("B")
    assert chosen == {"A", "B"}  # the planner itself took each of them somewhere


def test_compose_dispatch():
    """form A from 256 items on where three rows a lane fit the LDS budget, form B otherwise"""
    from genfer_amd import series

    for n, B, want in [(16, 1000, "A"), (16, 65, "B"), (40, 256, "A"), (40, 255, "B"), (64, 1000, "B"), (100, 1000, "B"), (32, 3, "B")]:
        series.compose(dev(dense((B, n), 5)), dev(dense((B, n), 6)))
        assert series.last_form() == want, (n, B)


# ---- no shortcuts, no neighbours, special values ------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,B", [(8, 300), (8, 7), (96, 7)])
def test_no_shortcuts_and_no_neighbours(n, B, oracle_lib):
    """rows on which subst_var or the product's dispatcher would shortcut get the general Horner loop, alone and inside a batch"""
    from genfer_amd import series

    F, G = dense((B, n), 77), dense((B, n), 78)
    G[0] = 0.0  # subst_var: a zero substitution
    G[1] = [0.0, 1.75] + [0.0] * (n - 2)  # ... a linear one with c = 0
    G[2] = [3.0] + [0.0] * (n - 1)  # a constant
    F[3, n - 1] = 0.0  # f with a zero leading coefficient: the first res is zero
    F[4, n - 1] = 1.0  # ... with a one
    G[5] = [1.0] + [0.0] * (n - 1)  # the product's y = 1
    F[6] = [2.0] + [0.0] * (n - 1)  # a constant f
    want = want_compose(oracle_lib, F, G, n)
    for form in ("A", "B"):
        series.set_form(form)
        batch = series.compose(dev(F), dev(G))
        assert_bits(batch, want, f"compose with shortcut rows, form {series.last_form()}")
        for b in range(7):  # each row alone == the row in the batch
            alone = series.compose(dev(F[b:b + 1]), dev(G[b:b + 1]))
            assert torch.equal(bits(alone), bits(batch[b:b + 1])), (form, b)
    series.set_form(None)


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
@pytest.mark.parametrize("nf,ng", [(8, 8), (8, 3), (3, 8), (8, 1), (1, 8)])
def test_special_values(form, nf, ng, oracle_lib):
    """inf, NaN, -0, subnormals and overflow in f and in g, every row against every row: the compact lengths keep a non-finite
    g[k] from meeting a padded zero, so a wrong loop bound shows as a NaN"""
    n = 8
    rows = special_rows(n)
    R = rows.shape[0]
    F = np.repeat(rows, R, axis=0)[:, :nf]
    G = np.tile(rows, (R, 1))[:, :ng]
    got, ran = run_compose(F, G, n, form)
    assert ran == form
    assert_bits(got, want_compose(oracle_lib, F, G, n), f"compose specials nf={nf} ng={ng} form {form}")


# ---- pow ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,nx,B", POW_SHAPES)
def test_pow_against_the_oracle_and_the_chain(n, nx, B, OTP, oracle_lib):
    from genfer_amd import series

    x = dense((B, nx), 700 * n + nx)
    X = dev(x)
    for e in POW_E:
        wo, wc = oracle_pow(OTP, x, e, n), want_pow(oracle_lib, x, e, n)
        for form in (None, "B"):
            series.set_form(form)
            got = series.pow(X, e, n=n)
            assert got.shape == (B, n)
            assert_bits(got, wo, f"pow n={n} nx={nx} B={B} e={e} form={form} vs the oracle")
            assert_bits(got, wc, f"pow n={n} nx={nx} B={B} e={e} form={form} vs the chain")
        series.set_form(None)
        # the explicit chain of series.mul calls on the same tensor
        res, base, ee = torch.ones((B, 1), dtype=torch.float64, device=DEV), X, e
        while ee > 0:
            if ee & 1:
                res = series.mul(res, base, n=min(res.shape[-1] + base.shape[-1] - 1, n))
            ee >>= 1
            if ee > 0:
                base = series.mul(base, base, n=min(2 * base.shape[-1] - 1, n))
        full = torch.zeros((B, n), dtype=torch.float64, device=DEV)
        full[:, :res.shape[-1]] = res
        assert torch.equal(bits(series.pow(X, e, n=n)), bits(full)), (n, nx, B, e)


def test_pow_special_values_and_views(oracle_lib):
    from genfer_amd import series

    n = 8
    x = special_rows(n)
    for e in (0, 1, 2, 3, 5):
        with np.errstate(all="ignore"):
            assert_bits(series.pow(dev(x), e), want_pow(oracle_lib, x, e, n), f"pow specials e={e}")
    # one constant series, no batch axes
    c = np.array([1.5])
    for e in (0, 1, 3):
        assert_bits(series.pow(dev(c), e, n=4), want_pow(oracle_lib, c[None], e, 4)[0], f"pow of a lone constant, e={e}")
    # one series for a whole batch, a sliced out with guards, in place
    x = dense((6, 5, 12), 91)
    want = want_pow(oracle_lib, x.reshape(30, 12), 5, 20).reshape(6, 5, 20)
    X = dev(x)
    xt = X.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert not xt.is_contiguous()
    assert_bits(series.pow(xt, 5, n=20), want, "pow permuted x")
    big = torch.full((6, 5, 25), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
    out = big[..., 2:22]
    assert series.pow(X, 5, n=20, out=out) is out
    assert_bits(out, want, "pow sliced out")
    g = big.view(torch.int64)
    assert bool((g[..., :2] == GUARD).all()) and bool((g[..., 22:] == GUARD).all())
    xe = X[0, 0].expand(6, 5, 12)
    assert_bits(series.pow(xe, 5, n=20), np.broadcast_to(want[0, 0], (6, 5, 20)).copy(), "pow expanded x")
    xi = X.clone()
    w12 = want_pow(oracle_lib, x.reshape(30, 12), 3, 12).reshape(6, 5, 12)
    assert series.pow(xi, 3, out=xi) is xi
    assert_bits(xi, w12, "pow in place")
    xi = X.clone()
    series.pow(xi, 0, out=xi)
    assert_bits(xi, want_pow(oracle_lib, x.reshape(30, 12), 0, 12).reshape(6, 5, 12), "pow e = 0 in place")


# ---- views -----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,batch", [(12, (5, 70)), (40, (3, 4, 6)), (130, (2, 5)), (20, (7,))])
def test_views(n, batch, oracle_lib):
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    B = int(np.prod(batch))
    nf = max(2, n // 2)
    f, g = dense((B, nf), 11), dense((B, n), 12)
    want = want_compose(oracle_lib, f, g, n).reshape(batch + (n,))
    F, G = dev(f).reshape(batch + (nf,)), dev(g).reshape(batch + (n,))
    # slices of wider tensors
    wide = torch.zeros(batch + (nf + 9,), dtype=torch.float64, device=DEV)
    wide[..., 4:4 + nf] = F
    fs = wide[..., 4:4 + nf]
    assert not fs.is_contiguous()
    assert_bits(series.compose(fs, G), want, "sliced f")
    # batch axes permuted
    if len(batch) >= 2:
        perm = tuple(reversed(range(len(batch))))
        gp = G.permute(*perm, len(batch)).contiguous().permute(*perm, len(batch))
        assert not gp.is_contiguous() and gp.stride(-1) == 1
        assert_bits(series.compose(F, gp), want, "permuted g")
        po = torch.empty(tuple(reversed(batch)) + (n,), dtype=torch.float64, device=DEV).permute(*perm, len(batch))
        series.compose(fs, gp, out=po)
        assert_bits(po, want, "permuted out")
    # a sliced out with guards around it, untouched
    big = torch.full(batch + (n + 5,), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
    out = big[..., 2:2 + n]
    assert series.compose(fs, G, out=out) is out
    assert_bits(out, want, "sliced out")
    gw = big.view(torch.int64)
    assert bool((gw[..., :2] == GUARD).all()) and bool((gw[..., 2 + n:] == GUARD).all())
    # one substitution into a whole batch (g with stride 0), and one f at a batch of points
    g0, f0 = g[:1], f[:1]
    ge = dev(g0).reshape((1,) * len(batch) + (n,)).expand(batch + (n,))
    assert ge.stride()[0] == 0
    assert_bits(series.compose(F, ge), want_compose(oracle_lib, f, np.repeat(g0, B, axis=0), n).reshape(batch + (n,)), "expanded g")
    assert_bits(series.compose(F, dev(g0)[0]), want_compose(oracle_lib, f, np.repeat(g0, B, axis=0), n).reshape(batch + (n,)), "broadcast 1-d g")
    assert_bits(series.compose(dev(f0)[0], G), want_compose(oracle_lib, np.repeat(f0, B, axis=0), g, n).reshape(batch + (n,)), "broadcast 1-d f")
    # in place over g, and over f (f as long as the result)
    ff = dense((B, n), 13)
    wf = want_compose(oracle_lib, ff, g, n).reshape(batch + (n,))
    for form in ("A", "B"):
        series.set_form(form)
        gi = G.clone()
        assert series.compose(F, gi, out=gi) is gi
        assert_bits(gi, want, f"compose in place over g, form {form}")
        fi = dev(ff).reshape(batch + (n,))
        assert series.compose(fi, G, out=fi) is fi
        assert_bits(fi, wf, f"compose in place over f, form {form}")
    series.set_form(None)
    # partial overlap
    buf = torch.zeros(batch + (2 * n,), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps g"):
        series.compose(F, buf[..., 0:n], out=buf[..., n // 2:n // 2 + n])
    with pytest.raises(TaylorError, match="partially overlaps f"):
        series.compose(buf[..., 1:n + 1], G, out=buf[..., 0:n])
    assert float((G + 1.0).sum().item()) > 0  # no stale HIP error


def test_long_rows_beside_the_lds_fallback(oracle_lib):
    """n = 4096 with a long g asks for more than 64 KB of LDS in form B (96 KB: two result rows and g)"""
    n, nf = 4096, 3
    f, g = dense((2, nf), 3), dense((2, n), 4)
    got, ran = run_compose(f, g, n)
    assert ran == "B"
    assert_bits(got, want_compose(oracle_lib, f, g, n), "compose n = 4096, ng = 4096")


def test_empty_batch_and_refusals():
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError
    import genfer_amd

    z = torch.zeros((0, 8), dtype=torch.float64, device=DEV)
    assert series.compose(z, z).shape == (0, 8) and series.pow(z, 3).shape == (0, 8)
    x = torch.rand((6, 16), dtype=torch.float64, device=DEV)
    y = torch.rand((6, 16), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="unit stride"):
        series.compose(torch.rand((6, 32), dtype=torch.float64, device=DEV)[:, ::2], y)
    with pytest.raises(TaylorError, match="zero stride"):
        series.compose(x, y, out=torch.empty((1, 16), dtype=torch.float64, device=DEV).expand(6, 16))
    with pytest.raises(TaylorError, match="partially overlaps x"):
        buf = torch.rand((6, 40), dtype=torch.float64, device=DEV)
        series.pow(buf[:, 0:16], 2, out=buf[:, 8:24])
    # through the C entry points
    series.last_form()  # declares them
    L = genfer_amd.lib()
    one = (C.c_size_t * 1)(6)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.gft_series_compose(vp(x), None, 16, vp(y), None, 16, vp(y), None, 0, one, 1, None) == -1
    assert "n == 0" in L.gft_last_error().decode()
    assert L.gft_series_compose(vp(x), None, 16, vp(y), None, 4, vp(y), None, 8, one, 1, None) == -1
    assert "nx = 16 > n = 8" in L.gft_last_error().decode()
    assert L.gft_series_pow(vp(x), None, 16, 3, vp(y), None, 4097, one, 1, None) == -1
    assert "4096" in L.gft_last_error().decode()
    assert L.gft_series_pow(vp(x), None, 16, 3, vp(y), None, 8, one, 1, None) == -1
    assert "nx = 16 > n = 8" in L.gft_last_error().decode()
    assert float((x + 1.0).sum().item()) > 0
    assert torch.equal(bits(series.compose(x, y)), bits(series.compose(x.clone(), y.clone())))


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
@pytest.mark.parametrize("op", ["compose", "pow"])
def test_stream_ordered_without_host_stall(which, op, oracle_lib):
    from genfer_amd import series

    B, n = 512, 24
    x, y = dense((B, n), 41), dense((B, n), 42)
    want = want_compose(oracle_lib, x, y, n) if op == "compose" else want_pow(oracle_lib, x, 5, n)
    X, Y = dev(x), dev(y)
    src = torch.zeros((B, n), dtype=torch.float64, device=DEV)
    call = (lambda t: series.compose(t, Y)) if op == "compose" else (lambda t: series.pow(t, 5))
    call(src)  # warm the kernels
    cycles = _sleep_cycles_for_ms(100)
    s = torch.cuda.Stream() if which == "side_stream" else torch.cuda.default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        src.copy_(X)  # the operand is produced behind a long kernel on this stream
        z = call(src)
        done = torch.cuda.Event()
        done.record()
        returned_early = not done.query()  # allowed to be false, never required
        twice = z * 2.0  # consumed right after, no host synchronisation in between
        src.zero_()  # the operand is reused right after
    s.synchronize()
    assert_bits(z, want, f"{op} on {which}")
    assert_bits(twice, want * 2.0, "consumer on " + which)
    assert returned_early in (True, False)


# ---- the handle API computes the same bits on the device ---------------------------------------------------------------------------


def test_agrees_with_the_handle_api():
    import genfer_amd
    from genfer_amd import series

    TP = genfer_amd.TaylorPoly
    B, n = 6, 48
    f, g = dense((B, n), 51), dense((B, n), 52)
    F, G = dev(f), dev(g)
    assert genfer_amd.lib().gft_set_conv_mode(3) == 0  # reference order
    try:
        zc = series.compose(F, G)
        zs = series.compose(F[:, :5], G[:, :7], n=n)
        zp = {e: series.pow(F, e) for e in (2, 5, 13)}
        for b in range(B):
            p, q = TP.from_torch(F[b]), TP.from_torch(G[b])
            assert torch.equal(bits(zc[b]), bits(p.subst_var(0, q).to_torch())), b
            ps, qs = TP.from_torch(F[b, :5], degrees_p1=(n,)), TP.from_torch(G[b, :7], degrees_p1=(n,))
            r = ps.subst_var(0, qs).to_torch()
            assert torch.equal(bits(zs[b, :r.shape[0]]), bits(r)) and not bool(zs[b, r.shape[0]:].any()), b
            for e, z in zp.items():
                assert torch.equal(bits(z[b]), bits(p.pow(e).to_torch())), (b, e)
    finally:
        assert genfer_amd.lib().gft_set_conv_mode(0) == 0
