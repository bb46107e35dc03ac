"""Batched bivariate compose and pow on device tensors (genfer_amd.series2.compose / pow, gft_series2_compose / gft_series2_pow) on
the MI355X.

Every coefficient of every item carries the bits of the chain of general products (tests/_series2_compose_cases.py, which
tests/test_series2_compose_cpu.py ties to the oracle's subst_var / pow and to the plain-Python model): both variables, both
instantiations of the compose kernel, compact operands, views, in-place results, special values and the stream contract."""
import numpy as np
import pytest

import _series2_compose_cases as cc
from _series2_oracle import assert_bits, compact_shapes, dense, signed

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 0x5A5A5A5A5A5A5A5A
CPU_BUDGET = 7.0e7  # B * nslices * (n0 * n1)^2 per case, tests/test_series2_gpu.py's budget: the chain stays within seconds

SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (8, 8), (16, 16), (5, 64), (64, 5), (9, 65)]
BATCHES = [1, 3, 65, 300]


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def compose(f, g, var, n=None, **kw):
    from genfer_amd import series, series2

    got = series2.compose(f if isinstance(f, torch.Tensor) else dev(f), g if isinstance(g, torch.Tensor) else dev(g), var, n=n, **kw)
    assert series.last_form() == "B"  # gft_series_last_form() == 2 after a series2 call
    return got


def power(x, e, n=None, **kw):
    from genfer_amd import series, series2

    got = series2.pow(x if isinstance(x, torch.Tensor) else dev(x), e, n=n, **kw)
    assert series.last_form() == "B"
    return got


# ---- compose: bit for bit against the chain ------------------------------------------------------------------------------------------


def compose_cases():
    for n in SHAPES:
        for var in (0, 1):
            for B in BATCHES:
                if B * n[var] * float(n[0] * n[1]) ** 2 <= CPU_BUDGET:
                    yield n, var, B


@pytest.mark.parametrize("var", [0, 1])
def test_compose_bit_exact(var, oracle_lib):
    """dense operands at every batch size the budget allows; compact and mixed-sign operands on the batches of 3 and 65"""
    checked = 0
    for n, v, B in compose_cases():
        if v != var:
            continue
        kinds = [("dense", n, n)]
        if B in (3, 65) and n != (1, 1):
            fs, gs = compact_shapes(*n)
            kinds += [("compact", fs, gs), ("signed", n, n)]
        for kind, fs, gs in kinds:
            make = signed if kind == "signed" else dense
            f, g = make((B,) + fs, 1000 * n[0] + n[1] + B), make((B,) + gs, 2000 * n[0] + n[1] + B + 7)
            assert_bits(compose(f, g, var, n), cc.want_compose(oracle_lib, f, g, var, n), f"compose var={var} n={n} B={B} {kind} f{fs} g{gs}")
            checked += 1
    assert checked >= 30


@pytest.mark.parametrize("n", [(3, 5), (8, 8), (16, 16)])
def test_compose_corners(n, oracle_lib):
    """one and two slices of f, g of stored shape (1, 1), (1, k), (k, 1), (2, 2), f shorter than n on the axis that stays"""
    B = 3
    for var in (0, 1):
        k = n[1 - var]  # the axis that stays
        slices = lambda s: (s, k) if var == 0 else (k, s)  # noqa: E731
        short = (n[0], max(1, n[1] // 2)) if var == 0 else (max(1, n[0] // 2), n[1])
        cases = [(slices(1), n), (slices(2), n), (short, n), (short, (2, 2))]
        cases += [(n, gs) for gs in [(1, 1), (1, n[1]), (n[0], 1), (2, 2), (1, 2), (2, 1)]]
        for fs, gs in cases:
            f, g = dense((B,) + fs, 300 * n[0] + fs[0] + var), dense((B,) + gs, 500 * n[1] + gs[1] + var)
            assert_bits(compose(f, g, var, n), cc.want_compose(oracle_lib, f, g, var, n), f"compose var={var} n={n} f{fs} g{gs}")
    # n defaults to the larger stored length on each axis
    f, g = dense((B, 2, n[1]), 5), dense((B, n[0], 2), 6)
    assert_bits(compose(f, g, 0), cc.want_compose(oracle_lib, f, g, 0, n), f"compose default n={n}")


@pytest.mark.parametrize("var", [0, 1])
def test_compose_both_instantiations(var, oracle_lib):
    """by construction: at (16, 16) the two result arrays and a dense g are 6 KB, resident under either grant; at (64, 64) the result
    arrays are 64 KB, so a g of (32, 64) (80 KB in all) is resident only under the 80 KB grant, and a g of (64, 64) (96 KB) stays
    in global memory whatever was granted.  f has 4 slices there: 3 steps, about 1e7 multiply-adds an item."""
    f, g = dense((5, 16, 16), 81), dense((5, 16, 16), 82)
    assert_bits(compose(f, g, var), cc.want_compose(oracle_lib, f, g, var, (16, 16)), "compose (16, 16), g resident")
    n = (64, 64)
    fs = (4, 64) if var == 0 else (64, 4)
    f = dense((2,) + fs, 83)
    for gs in [(64, 64), (32, 64)]:
        g = signed((2,) + gs, 84)
        assert_bits(compose(f, g, var, n), cc.want_compose(oracle_lib, f, g, var, n), f"compose var={var} n={n} f{fs} g{gs}")
    # g in global memory through a row stride of its own
    wide = torch.zeros((2, 64, 80), dtype=torch.float64, device=DEV)
    wide[..., 3:67] = dev(dense((2, 64, 64), 85))
    gv = wide[..., 3:67]
    assert gv.stride(-2) == 80
    assert_bits(compose(f, gv, var, n), cc.want_compose(oracle_lib, f, gv.cpu().numpy(), var, n), f"compose var={var} n={n}, strided g in global memory")


@pytest.mark.parametrize("n,batch", [((3, 5), (4, 5)), ((9, 17), (2, 3)), ((16, 16), (7,))])
def test_compose_views(n, batch, oracle_lib):
    B, nb = int(np.prod(batch)), len(batch)
    f, g = dense((B,) + n, 11), dense((B,) + n, 12)
    expect = {var: cc.want_compose(oracle_lib, f, g, var, n).reshape(batch + n) for var in (0, 1)}
    F, G = dev(f).reshape(batch + n), dev(g).reshape(batch + n)
    # row-strided operands: slices of wider tensors on both series axes
    wide = torch.zeros(batch + (n[0] + 3, n[1] + 9), dtype=torch.float64, device=DEV)
    wide[..., 1:1 + n[0], 4:4 + n[1]] = F
    fv = wide[..., 1:1 + n[0], 4:4 + n[1]]
    wide_g = torch.zeros(batch + (n[0] + 1, n[1] + 2), dtype=torch.float64, device=DEV)
    wide_g[..., 1:, 2:] = G
    gv = wide_g[..., 1:, 2:]
    assert not fv.is_contiguous() and fv.stride(-2) == n[1] + 9 and gv.stride(-2) == n[1] + 2
    for var in (0, 1):
        assert_bits(compose(fv, gv, var), expect[var], f"compose var={var} sliced f and g")
    # a transposed batch
    if nb >= 2:
        perm = tuple(reversed(range(nb))) + (nb, nb + 1)
        fp = F.permute(*perm).contiguous().permute(*perm)
        assert not fp.is_contiguous() and fp.stride(-1) == 1
        po = torch.empty(tuple(reversed(batch)) + n, dtype=torch.float64, device=DEV).permute(*perm)
        for var in (0, 1):
            assert_bits(compose(fp, G, var), expect[var], f"compose var={var} permuted f")
            assert compose(F, G, var, out=po) is po
            assert_bits(po, expect[var], f"compose var={var} permuted out")
    # a non-contiguous out with guard words around it, intact afterwards
    for var in (0, 1):
        big = torch.full(batch + (n[0] + 2, n[1] + 5), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
        out = big[..., 1:1 + n[0], 2:2 + n[1]]
        assert compose(fv, G, var, out=out) is out
        assert_bits(out, expect[var], f"compose var={var} sliced out")
        w = big.view(torch.int64).clone()
        w[..., 1:1 + n[0], 2:2 + n[1]] = GUARD
        assert bool((w == GUARD).all()), var
    # one g for the whole batch: stride 0, expanded and broadcast; one f against many g
    g0 = np.repeat(g[:1], B, axis=0)
    ge = dev(g[:1]).reshape((1,) * nb + n).expand(batch + n)
    assert ge.stride(0) == 0
    for var in (0, 1):
        want0 = cc.want_compose(oracle_lib, f, g0, var, n).reshape(batch + n)
        assert_bits(compose(F, ge, var), want0, f"compose var={var} expanded g")
        assert_bits(compose(F, dev(g[0]), var), want0, f"compose var={var} broadcast g")
        assert_bits(compose(dev(f[0]), G, var), cc.want_compose(oracle_lib, np.repeat(f[:1], B, axis=0), g, var, n).reshape(batch + n),
                    f"compose var={var} broadcast f")
    # in place: out is f, out is g, out is a strided view of f
    for var in (0, 1):
        fi = F.clone()
        assert compose(fi, G, var, out=fi) is fi
        assert_bits(fi, expect[var], f"compose var={var} in place on f")
        gi = G.clone()
        compose(F, gi, var, out=gi)
        assert_bits(gi, expect[var], f"compose var={var} in place on g")
        wi = wide.clone()
        v = wi[..., 1:1 + n[0], 4:4 + n[1]]
        compose(v, G, var, out=v)
        assert_bits(v, expect[var], f"compose var={var} in place on a sliced f")


def test_compose_in_place_with_g_in_global_memory(oracle_lib):
    """at (64, 64) with a dense g the kernel reads g from global memory in every step: the result may still be g, or f"""
    n = (64, 64)
    f, g = dense((2,) + n, 91), signed((2,) + n, 92)
    f[:, 3:, :] = 0.0  # (the chain is the expected value whatever f holds; zeros keep the magnitudes down)
    want = cc.want_compose(oracle_lib, f, g, 0, n)
    gi = dev(g)
    compose(dev(f), gi, 0, out=gi)
    assert_bits(gi, want, "compose in place on a g in global memory")
    fi = dev(f)
    compose(fi, dev(g), 0, out=fi)
    assert_bits(fi, want, "compose in place on f, g in global memory")


def test_empty_batch_is_a_no_op():
    from genfer_amd import series2

    e = torch.zeros((0, 3, 8), dtype=torch.float64, device=DEV)
    assert series2.compose(e, e).shape == (0, 3, 8) and series2.compose(e, e, 1).shape == (0, 3, 8)
    assert series2.pow(e, 3).shape == (0, 3, 8) and series2.pow(e, 0).shape == (0, 3, 8)


INF, NAN = float("inf"), float("nan")


def test_special_values():
    """infinities, NaNs, exact zeros and negative zeros follow the plain-Python model bit for bit (a NaN for a NaN), and an item does
    not change its neighbour in the batch"""
    n = (4, 5)
    plain = dense(n, 71)
    items = []
    for (i, j, v) in [(1, 1, INF), (0, 2, -INF), (2, 0, NAN), (3, 4, INF)]:
        a = plain.copy()
        a[i, j] = v
        items.append(a)
    z = plain.copy()
    z[1:, :] = 0.0
    z[0, 2:] = -0.0
    items += [z, -z, np.where(np.eye(*n) > 0, 1.0, np.where(plain > 1.0, -0.0, 0.0)), plain]
    f = np.stack(items)
    g = np.stack(items[::-1])
    for var in (0, 1):
        got = compose(f, g, var, n)
        assert_bits(got, np.stack([cc.model_compose(f[b], g[b], var, n) for b in range(len(items))]), f"compose var={var} specials")
        alone = compose(f[-1:], g[-1:], var, n)
        assert torch.equal(alone.view(torch.int64), got[-1:].view(torch.int64)), "the plain item inside the batch of specials"
        # one slice: 0.0 + f, and g's values (NaNs among them) are not used
        one = -z[None, :1] if var == 0 else -z[None, :, :1]
        got = compose(np.repeat(one, len(items), axis=0), g, var, n)
        assert_bits(got, np.repeat(cc.pad2(0.0 + one[0], n)[None], len(items), axis=0), f"compose var={var} one slice")
        # g of stored shape (1, 1): a constant, zero and negative zero included
        for c in (0.75, 0.0, -0.0, INF):
            gc = np.full((len(items), 1, 1), c)
            assert_bits(compose(f, gc, var, n), np.stack([cc.model_compose(f[b], gc[b], var, n) for b in range(len(items))]),
                        f"compose var={var} g = [[{c}]]")
    for e in (0, 1, 2, 3, 5):
        assert_bits(power(f, e, n), np.stack([cc.model_pow(f[b], e, n) for b in range(len(items))]), f"pow e={e} specials")


# ---- pow -----------------------------------------------------------------------------------------------------------------------------

POW_E = [0, 1, 2, 3, 5, 8, 13, 31]


@pytest.mark.parametrize("n,B", [((8, 8), 300), ((16, 16), 65), ((5, 64), 3), ((64, 64), 1)])
def test_pow_bit_exact(n, B, oracle_lib):
    """dense and compact x, and out= in place"""
    xd = dense((B,) + n, 700 * n[0] + n[1])
    xc = dense((B,) + compact_shapes(*n)[0], 900 * n[0] + n[1])
    if n == (64, 64):  # |x| < 1 around a constant term of 1: x^31 stays far from overflow at 4096 coefficients
        xd, xc = (xd - 0.5) / 64.0, (xc - 0.5) / 64.0
        xd[:, 0, 0] = xc[:, 0, 0] = 1.0
    for e in POW_E:
        assert_bits(power(xd, e, n), cc.want_pow(oracle_lib, xd, e, n), f"pow n={n} B={B} e={e} dense")
        assert_bits(power(xc, e, n), cc.want_pow(oracle_lib, xc, e, n), f"pow n={n} B={B} e={e} compact x{xc.shape[1:]}")
    for e in (0, 1, 5):
        xi = dev(xd)
        assert power(xi, e, out=xi) is xi
        assert_bits(xi, cc.want_pow(oracle_lib, xd, e, n), f"pow n={n} B={B} e={e} in place")


def test_pow_views(oracle_lib):
    """a row-strided x under a multi-axis batch, a broadcast x, and a sliced out with guard words around it"""
    n, batch = (5, 9), (2, 3)
    x = dense((6,) + n, 21)
    want = cc.want_pow(oracle_lib, x, 5, n).reshape(batch + n)
    wide = torch.zeros(batch + (n[0] + 2, n[1] + 7), dtype=torch.float64, device=DEV)
    wide[..., 2:, 3:3 + n[1]] = dev(x).reshape(batch + n)
    xv = wide[..., 2:, 3:3 + n[1]]
    assert xv.stride(-2) == n[1] + 7
    assert_bits(power(xv, 5), want, "pow sliced x")
    big = torch.full(batch + (n[0] + 2, n[1] + 5), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
    out = big[..., 1:1 + n[0], 2:2 + n[1]]
    for e in (0, 5):
        assert power(xv, e, out=out) is out
        assert_bits(out, cc.want_pow(oracle_lib, x, e, n).reshape(batch + n), f"pow e={e} sliced out")
        w = big.view(torch.int64).clone()
        w[..., 1:1 + n[0], 2:2 + n[1]] = GUARD
        assert bool((w == GUARD).all()), e
    xe = dev(x[0]).expand(batch + n)
    assert_bits(power(xe, 3, out=torch.empty(batch + n, dtype=torch.float64, device=DEV)),
                cc.want_pow(oracle_lib, np.repeat(x[:1], 6, axis=0), 3, n).reshape(batch + n), "pow expanded x")
    v = wide.clone()[..., 2:, 3:3 + n[1]]
    power(v, 5, out=v)
    assert_bits(v, want, "pow in place on a sliced x")


# ---- refusals through the C entry points -----------------------------------------------------------------------------------------------


def test_refusals():
    import ctypes as C

    import genfer_amd
    from genfer_amd import series2
    from genfer_amd.taylor import TaylorError

    x = torch.rand((6, 4, 16), dtype=torch.float64, device=DEV) + 0.5
    y = torch.rand((6, 4, 16), dtype=torch.float64, device=DEV) + 0.5
    buf = torch.rand((6, 4, 40), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps f"):
        series2.compose(buf[..., 0:16], y, out=buf[..., 8:24])
    with pytest.raises(TaylorError, match="partially overlaps g"):
        series2.compose(x, buf[..., 0:16], 1, out=buf[..., 16:32])
    with pytest.raises(TaylorError, match="partially overlaps x"):
        series2.pow(buf[..., 0:16], 2, out=buf[..., 8:24])
    with pytest.raises(TaylorError, match="zero stride"):
        series2.pow(x, 2, out=torch.empty((1, 4, 16), dtype=torch.float64, device=DEV).expand(6, 4, 16))
    series2.compose(x, y)  # declares the entry points
    L = genfer_amd.lib()
    one = (C.c_size_t * 1)(6)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = torch.zeros((6, 4, 16), dtype=torch.float64, device=DEV)
    for var in (2, -1):
        assert L.gft_series2_compose(vp(x), None, 16, 4, 16, vp(y), None, 16, 4, 16, var, vp(out), None, 16, 4, 16, one, 1, None) == -1
        assert f"var = {var}" in L.gft_last_error().decode()
    assert L.gft_series2_compose(vp(x), None, 16, 4, 16, vp(y), None, 16, 4, 16, 1, vp(out), None, 16, 3, 16, one, 1, None) == -1
    assert "longer than the truncation order" in L.gft_last_error().decode()
    assert L.gft_series2_pow(vp(x), None, 16, 4, 16, 3, vp(out), None, 16, 17, 241, one, 1, None) == -1
    assert "exceeds the limit of 4096" in L.gft_last_error().decode()
    assert L.gft_series2_pow(vp(x), None, 16, 4, 16, 3, vp(out), None, 16, 4, 16, one, 1, None) == 0
    assert float((x + 1.0).sum().item()) > 0  # no stale HIP error: torch's next call succeeds
    assert torch.equal(out.view(torch.int64), series2.pow(x, 3).view(torch.int64))


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
    from genfer_amd import series2

    B, n = 512, (4, 6)
    x, y = dense((B,) + n, 41), dense((B,) + n, 42)
    want_c, want_p = cc.want_compose(oracle_lib, x, y, 1, n), cc.want_pow(oracle_lib, x, 5, n)
    X, Y = dev(x), dev(y)
    src = torch.zeros((B,) + n, dtype=torch.float64, device=DEV)
    series2.compose(src, Y, 1)  # warm the kernels
    series2.pow(src, 5)
    cycles = _sleep_cycles_for_ms(100)
    s = torch.cuda.Stream() if which == "side_stream" else torch.cuda.default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        src.copy_(X)  # the operand is produced behind a long kernel on this stream
        c = series2.compose(src, Y, 1)
        p = series2.pow(src, 5)
        done = torch.cuda.Event()
        done.record()
        returned_early = not done.query()  # allowed to be false, never required
        twice = c * 2.0 + p  # consumed right after, no host synchronisation in between
        src.zero_()  # the operand is reused right after
    s.synchronize()
    assert_bits(c, want_c, "compose on " + which)
    assert_bits(p, want_p, "pow on " + which)
    assert_bits(twice, want_c * 2.0 + want_p, "consumer on " + which)
    assert returned_early in (True, False)
