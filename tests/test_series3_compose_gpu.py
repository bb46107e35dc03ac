"""compose and pow of the batched trivariate series (genfer_amd.series3, gft_series3_compose / gft_series3_pow) on the MI355X.

Every coefficient of every item carries the bits of the chain of series3.mul's products that defines the operation
(tests/_series3_compose_cases.py: orc_mul_raw at rank 3, which tests/test_series3_compose_cpu.py ties to the oracle's own subst_var /
pow and to the plain-Python model); a NaN matches a NaN.  The squeeze and its sentinels, both forms of the kernel (g in LDS, g in
global memory), views, in-place results, special values, shortcut operands, refusals and the stream contract."""
import ctypes as C

import numpy as np
import pytest

import _series3_compose_cases as cc
from _series3_oracle import assert_bits, bits_equal, dense, signed

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 0x5A5A5A5A5A5A5A5A
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64)


def compose(f, g, var, n=None, **kw):
    from genfer_amd import series, series3

    got = series3.compose(f if isinstance(f, torch.Tensor) else dev(f), g if isinstance(g, torch.Tensor) else dev(g), var=var, n=n, **kw)
    assert series.last_form() == "B"  # gft_series_last_form() == 2 after a series3 call
    return got


def power(x, e, n=None, **kw):
    from genfer_amd import series, series3

    got = series3.pow(x if isinstance(x, torch.Tensor) else dev(x), e, n=n, **kw)
    assert series.last_form() == "B"
    return got


def small_g(shape, seed, B=None):
    """a dense g whose coefficients sum to about one: the Horner values stay finite over hundreds of steps"""
    return dense(((B,) if B else ()) + tuple(shape), seed) / float(np.prod(shape))


# ---- compose against the chain ---------------------------------------------------------------------------------------------------

# the smallest item with no unit axis; asymmetric; the one-wave boundary (64 and 72 output pairs); several waves; a long axis, whose
# loop has 512 steps along it; the limit
SHAPES = [(2, 2, 2), (3, 4, 5), (5, 3, 2), (4, 4, 8), (4, 4, 9), (8, 8, 8), (2, 2, 513), (16, 16, 16)]
BATCHES = [1, 3, 65, 300]
CPU_BUDGET = 7.0e7  # B * (n0 * n1 * n2)^2 per case, test_series3_gpu.py's rule: the oracle side stays within seconds


def cases():
    for n in SHAPES:
        N = n[0] * n[1] * n[2]
        for B in BATCHES:
            if N == 4096 and B != 3 or B > 3 and B * float(N) ** 2 > CPU_BUDGET:
                continue
            yield n, B


def forms(n, var, B):
    """(f shape, g shape): a full f and g at every batch; at B = 3 also g compact (2, 2, 2), with one and with two unit axes, and a
    compact, a two-slice and a one-slice f; at the limit g of 2048 coefficients (the largest that sits in LDS under an 80 KB grant)
    and of 2304 (the global form)"""
    out = [(n, n)]
    if B == 3:
        out += [(n, tuple(min(2, v) for v in n)), (n, (1, n[1], n[2])), (n, (n[0], 1, 1)),
                (cc.compact_shapes(n)[0], n), (cc.two_slices(n, var), n), (tuple(1 if a == var else n[a] for a in range(3)), n)]
        if n == (16, 16, 16):
            out += [(n, (16, 16, 8)), (n, (16, 16, 9))]
    return out


@pytest.mark.parametrize("var", [0, 1, 2])
def test_compose_bit_exact_against_the_chain(var, oracle_lib):
    checked = 0
    for n, B in cases():
        for fs, gs in forms(n, var, B):
            f = dense((B,) + fs, 1000 * n[0] + 10 * n[1] + n[2] + B + var)
            g = small_g(gs, 2000 * n[0] + 10 * n[1] + n[2] + B + 7, B)
            got = compose(f, g, var, n)
            assert_bits(got, cc.want_compose(oracle_lib, f, g, var, n), f"compose var={var} n={n} B={B} f{fs} g{gs}")
            checked += 1
    assert checked == 26 + 8 * 6 + 2  # 26 (n, B); six more forms at B = 3 of each of the 8 shapes; two at the limit


# ---- the squeeze -----------------------------------------------------------------------------------------------------------------

SQUEEZES = [(3, 1, 4), (3, 4, 1), (1, 3, 4), (4, 1, 1), (1, 1, 5), (1, 1, 1)]
# stored unit axes under longer result axes: S differs from n
THIN = [((2, 2, 1), (2, 1, 1), (4, 3, 2)), ((1, 3, 2), (2, 1, 2), (3, 3, 3)), ((3, 1, 1), (1, 1, 2), (3, 2, 4)), ((2, 3, 2), (1, 1, 1), (3, 3, 3))]


def test_sentinels_of_the_squeeze(oracle_lib):
    """the device carries the chain's bits where a product in the caller's axis order without the squeeze does not"""
    for fs, gs, n, var in cc.SENTINELS:
        for kind in (dense, signed):
            f, g = np.stack([kind(fs, 3), kind(fs, 5)]), np.stack([kind(gs, 4), kind(gs, 6)])
            got = compose(f, g, var, n).cpu().numpy()
            assert_bits(got, cc.want_compose(oracle_lib, f, g, var, n), f"sentinel f{fs} g{gs} n={n} var={var}")
            assert not bits_equal(got[0], cc.unsqueezed_compose(f[0], g[0], var, n)).all(), (fs, gs, n, var)


def test_squeezed_result_shapes(oracle_lib):
    checked = differs = 0
    for fs, gs, n in [(n, n, n) for n in SQUEEZES] + THIN:
        for var in (0, 1, 2):
            f, g = dense((3,) + fs, 100 * n[0] + sum(fs) + var), dense((3,) + gs, 200 * n[1] + sum(gs))
            got = compose(f, g, var, n)
            assert_bits(got, cc.want_compose(oracle_lib, f, g, var, n), f"compose f{fs} g{gs} n={n} var={var}")
            s = cc.step_shapes(fs, gs, n, var)[-1]
            differs += s != n
            outside = got.cpu().numpy().copy()
            outside[:, :s[0], :s[1], :s[2]] = 0.0
            assert not outside.any() and not np.signbit(outside).any(), (fs, gs, n, var, "outside the stored shape is +0.0")
            checked += 1
    assert checked == 30 and differs >= 8


# ---- pow against the chain -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [(3, 4, 5), (4, 4, 9)])
def test_pow_bit_exact_against_the_chain(n, oracle_lib):
    checked = 0
    for e in cc.POW_E:
        for B, xs in [(3, n), (65, n), (3, cc.compact_shapes(n)[0]), (3, (n[0], 1, n[2])), (3, (1, 1, n[2]))]:
            x = dense((B,) + xs, 50 * n[0] + n[2] + e + B)
            assert_bits(power(x, e, n), cc.want_pow(oracle_lib, x, e, n), f"pow e={e} n={n} B={B} x{xs}")
            checked += 1
    assert checked == 35


def test_pow_edges(oracle_lib):
    n = (16, 16, 16)
    x = dense((3,) + n, 91) / 64.0
    assert_bits(power(x, 5, n), cc.want_pow(oracle_lib, x, 5, n), "pow e=5 at the limit")
    # e = 1 runs the loop: 0.0 + 1.0 * x, so -0.0 becomes +0.0
    x = dense((2, 3, 4, 5), 92)
    x[0, 1, 2, 3] = x[1, 0, 0, 0] = -0.0
    got = power(x, 1)
    assert_bits(got, cc.want_pow(oracle_lib, x, 1, (3, 4, 5)), "pow e=1 on an item holding -0.0")
    assert_bits(got, 0.0 + x, "pow e=1 is 0.0 + x")
    assert not np.signbit(got.cpu().numpy()).any()
    # e = 0: the unit item, into a larger n, whatever x holds
    x = np.full((3, 2, 2, 2), NAN)
    unit = np.zeros((3, 4, 3, 5))
    unit[:, 0, 0, 0] = 1.0
    assert_bits(power(x, 0, (4, 3, 5)), unit, "pow e=0 into a larger n")
    assert_bits(power(dense((3, 2, 2, 2), 93), 3, (4, 3, 5)), cc.want_pow(oracle_lib, dense((3, 2, 2, 2), 93), 3, (4, 3, 5)), "pow into a larger n")


# ---- views -----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,batch,var", [((3, 4, 5), (4, 5), 0), ((4, 4, 9), (2, 3), 1), ((3, 4, 5), (2, 3), 2)])
def test_views(n, batch, var, oracle_lib):
    from genfer_amd import series3

    B, nb = int(np.prod(batch)), len(batch)
    f, g = dense((B,) + n, 11), small_g(n, 12, B)
    wc = cc.want_compose(oracle_lib, f, g, var, n).reshape(batch + n)
    wp = cc.want_pow(oracle_lib, f, 5, n).reshape(batch + n)
    F, G = dev(f).reshape(batch + n), dev(g).reshape(batch + n)

    def sliced(t, fill=0.0):
        wide = torch.full(batch + (n[0] + 2, n[1] + 3, n[2] + 9), fill, dtype=torch.float64, device=DEV)
        wide[..., 1:1 + n[0], 2:2 + n[1], 4:4 + n[2]] = t
        v = wide[..., 1:1 + n[0], 2:2 + n[1], 4:4 + n[2]]
        assert not v.is_contiguous() and v.stride(-2) == n[2] + 9 and v.stride(-3) == (n[1] + 3) * (n[2] + 9)
        return v

    # f and g as slices of wider tensors on all three series axes
    fv, gv = sliced(F), sliced(G)
    assert_bits(series3.compose(fv, gv, var=var), wc, "compose sliced f and g")
    assert_bits(series3.pow(fv, 5), wp, "pow sliced x")
    # out as such a slice, guard words intact around it
    for call, want, what in [(lambda o: series3.compose(fv, gv, var=var, out=o), wc, "compose"), (lambda o: series3.pow(fv, 5, out=o), wp, "pow")]:
        big = torch.full(batch + (n[0] + 2, n[1] + 2, n[2] + 5), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
        out = big[..., 1:1 + n[0], 1:1 + n[1], 2:2 + n[2]]
        assert call(out) is out
        assert_bits(out, want, f"{what} sliced out")
        w = big.view(torch.int64).clone()
        w[..., 1:1 + n[0], 1:1 + n[1], 2:2 + n[2]] = GUARD
        assert bool((w == GUARD).all()), what
    # a permuted batch
    perm = tuple(reversed(range(nb))) + (nb, nb + 1, nb + 2)
    fp = F.permute(*perm).contiguous().permute(*perm)
    assert not fp.is_contiguous() and fp.stride(-1) == 1
    assert_bits(series3.compose(fp, G, var=var), wc, "compose permuted f")
    assert_bits(series3.pow(fp, 5), wp, "pow permuted x")
    # one g for the whole batch: batch stride 0, and a plain [ng0, ng1, ng2] tensor
    w1 = cc.want_compose(oracle_lib, f, g[0], var, n).reshape(batch + n)
    ge = dev(g[:1]).reshape((1,) * nb + n).expand(batch + n)
    assert ge.stride(0) == 0
    assert_bits(series3.compose(F, ge, var=var), w1, "compose expanded g")
    assert_bits(series3.compose(F, dev(g[0]), var=var), w1, "compose one g")
    # slab and row strides of 0: a row repeated through the item
    frep = np.broadcast_to(f[:, :1, :1], f.shape).copy()
    fr = dev(f[:, :1, :1]).reshape(batch + (1, 1, n[2])).expand(batch + n)
    assert fr.stride(-2) == 0 and fr.stride(-3) == 0
    assert_bits(series3.compose(fr, G, var=var), cc.want_compose(oracle_lib, frep, g, var, n).reshape(batch + n), "compose f with strides of 0")
    gr = dev(f[:, :1, :1] / 64.0).reshape(batch + (1, 1, n[2])).expand(batch + n)
    assert gr.stride(-2) == 0 and gr.stride(-3) == 0
    assert_bits(series3.compose(F, gr, var=var), cc.want_compose(oracle_lib, f, frep / 64.0, var, n).reshape(batch + n), "compose g with strides of 0")
    assert_bits(series3.pow(fr, 5), cc.want_pow(oracle_lib, frep, 5, n).reshape(batch + n), "pow x with strides of 0")
    # in place: compose on f and on g, pow on x; contiguous and through a sliced view
    for make in (lambda t: t.clone(), lambda t: sliced(t, 7.0)):
        fi = make(F)
        assert series3.compose(fi, G, var=var, out=fi) is fi
        assert_bits(fi, wc, "compose in place on f")
        gi = make(G)
        series3.compose(F, gi, var=var, out=gi)
        assert_bits(gi, wc, "compose in place on g")
        xi = make(F)
        series3.pow(xi, 5, out=xi)
        assert_bits(xi, wp, "pow in place on x")


def test_default_orders_and_empty_batch(oracle_lib):
    from genfer_amd import series3

    f, g = dense((5, 3, 2, 6), 61), small_g((2, 4, 2), 62, 5)
    for var in (0, 1, 2):
        assert_bits(series3.compose(dev(f), dev(g), var=var), cc.want_compose(oracle_lib, f, g, var, (3, 4, 6)), f"compose default n var={var}")
    assert_bits(series3.compose(dev(f), dev(g)), cc.want_compose(oracle_lib, f, g, 0, (3, 4, 6)), "compose default var")
    assert_bits(series3.pow(dev(f), 3), cc.want_pow(oracle_lib, f, 3, (3, 2, 6)), "pow default n")
    e = torch.zeros((0, 3, 2, 8), dtype=torch.float64, device=DEV)
    assert series3.compose(e, e, var=1).shape == (0, 3, 2, 8) and series3.pow(e, 3).shape == (0, 3, 2, 8) and series3.pow(e, 0).shape == (0, 3, 2, 8)


# ---- special values and shortcut operands ------------------------------------------------------------------------------------------


def model_compose_batch(f, g, var, n):
    return np.stack([cc.model_compose(f[b], g[b], var, n) for b in range(f.shape[0])])


def test_special_values():
    """infinities, NaNs, exact zeros and negative zeros follow the definition bit for bit (a NaN for a NaN)"""
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
    f = np.stack(items)
    g = np.stack(items[::-1])
    with np.errstate(all="ignore"):
        for var in (0, 1, 2):
            got = compose(f, g, var, n)
            assert_bits(got, model_compose_batch(f, g, var, n), f"compose specials var={var}")
            alone = compose(f[-1:], g[-1:], var, n)
            assert torch.equal(bits(alone), bits(got[-1:])), (var, "the plain item inside the batch of specials")
        for e in (1, 2, 5):
            got = power(f, e, n)
            assert_bits(got, np.stack([cc.model_pow(f[b], e, n) for b in range(f.shape[0])]), f"pow specials e={e}")
            assert torch.equal(bits(power(f[-1:], e, n)), bits(got[-1:])), (e, "the plain item inside the batch of specials")


def test_shortcut_operands_take_the_general_loops():
    """zero, one, constant and linear g (and f) -- what subst_var and Mul shortcut -- give the general loops, and every item alone
    equals the item inside the batch"""
    n = (3, 3, 3)
    plain = dense(n, 81)
    zero, one, const, lin = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    one[0, 0, 0] = 1.0
    const[0, 0, 0] = 2.5
    lin[0, 0, 0], lin[0, 0, 1], lin[1, 0, 0] = 1.5, 0.75, -0.5
    var1 = np.zeros(n)
    var1[0, 1, 0] = 1.0  # the variable itself
    g = np.stack([zero, one, const, lin, var1, plain, plain, plain])
    f = np.stack([plain, plain, plain, plain, plain, zero, const, lin])
    with np.errstate(all="ignore"):
        for var in (0, 1, 2):
            got = compose(f, g, var, n)
            assert_bits(got, model_compose_batch(f, g, var, n), f"compose shortcut operands var={var}")
            for b in range(f.shape[0]):
                assert torch.equal(bits(compose(f[b:b + 1], g[b:b + 1], var, n)), bits(got[b:b + 1])), (var, b)
        # a g stored as one coefficient: the constant as a shape
        gc = dense((8, 1, 1, 1), 82)
        for var in (0, 1, 2):
            assert_bits(compose(f, gc, var, n), model_compose_batch(f, gc, var, n), f"compose g of one coefficient var={var}")
        x = np.stack([zero, one, const, lin, plain])
        for e in (0, 1, 3, 8):
            got = power(x, e, n)
            assert_bits(got, np.stack([cc.model_pow(x[b], e, n) for b in range(x.shape[0])]), f"pow shortcut operands e={e}")
            for b in range(x.shape[0]):
                assert torch.equal(bits(power(x[b:b + 1], e, n)), bits(got[b:b + 1])), (e, b)


# ---- refusals through the C entry points -----------------------------------------------------------------------------------------


def test_c_entry_point_refusals(oracle_lib):
    from genfer_amd import series3
    import genfer_amd

    f = torch.rand((6, 2, 4, 16), dtype=torch.float64, device=DEV) + 0.5
    gbuf = (torch.rand(3 * 768, dtype=torch.float64, device=DEV) + 0.5) / 128.0
    g = gbuf[768:1536].view(6, 2, 4, 16)  # (inside a wider buffer: a result that starts in g overlaps nothing else)

    def after():  # no stale HIP error: torch's next call succeeds
        assert float((f + 1.0).sum().item()) > 0

    good = series3.compose(f, g, var=1)  # declares the entry points
    L = genfer_amd.lib()
    one = (C.c_size_t * 1)(6)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    big = torch.zeros(6 * 4097, dtype=torch.float64, device=DEV)

    def c_compose(nf, ng, nr, var=1, rss=None, rrs=None, fss=64, res=big):
        return L.gft_series3_compose(vp(f), None, fss, 16, *nf, vp(g), None, 64, 16, *ng, var, None if res is None else vp(res), None,
                                     nr[1] * nr[2] if rss is None else rss, nr[2] if rrs is None else rrs, *nr, one, 1, None)

    def c_pow(nx, nr, e=5, res=big, rss=None):
        return L.gft_series3_pow(vp(f), None, 64, 16, *nx, e, None if res is None else vp(res), None, nr[1] * nr[2] if rss is None else rss,
                                 nr[2], *nr, one, 1, None)

    full = (2, 4, 16)
    for args, kw, text in [((full, full, full), {"var": 3}, "series3_compose: var = 3 (the variable of f that g replaces is 0, 1 or 2)"),
                           ((full, full, full), {"var": -1}, "series3_compose: var = -1"),
                           ((full, full, full), {"res": None}, "series3_compose: the result is a null pointer"),
                           ((full, full, full), {"rrs": -16}, "negative strides"),
                           ((full, full, full), {"fss": -64}, "negative strides are not supported (f, the slab axis)"),
                           ((full, full, full), {"rss": 0}, "zero slab stride"),
                           ((full, full, full), {"rrs": 0}, "zero row stride"),
                           ((full, full, full), {"rss": 32}, "overlap each other"),
                           ((full, full, full), {"res": f[0, 0, 1]}, "series3_compose: the result partially overlaps f"),
                           ((full, full, full), {"res": gbuf[768 + 64:]}, "series3_compose: the result partially overlaps g"),
                           ((full, full, (17, 241, 1)), {}, "n0 * n1 * n2 = 17 * 241 * 1 exceeds the limit of 4096"),
                           ((full, full, (2, 3, 16)), {}, "f has 2 x 4 x 16 coefficients, the result 2 x 3 x 16"),
                           ((full, (2, 4, 0), full), {}, "an operand has no coefficients")]:
        assert c_compose(*args, **kw) == -1 and text in L.gft_last_error().decode(), (text, L.gft_last_error())
        after()
    for args, kw, text in [((full, full), {"res": None}, "series3_pow: the result is a null pointer"),
                           ((full, full), {"rss": 0}, "zero slab stride"),
                           ((full, full), {"res": f[0, 0, 1]}, "series3_pow: the result partially overlaps x"),
                           ((full, (17, 241, 1)), {}, "n0 * n1 * n2 = 17 * 241 * 1 exceeds the limit of 4096"),
                           ((full, (2, 3, 16)), {}, "x has 2 x 4 x 16 coefficients, the result 2 x 3 x 16")]:
        assert c_pow(*args, **kw) == -1 and text in L.gft_last_error().decode(), (text, L.gft_last_error())
        after()
    # a good call still runs, through the C entry point and through the module
    assert c_compose(full, full, full) == 0 and L.gft_series_last_form() == 2
    after()
    assert torch.equal(bits(big[:6 * 128].reshape(6, 2, 4, 16)), bits(good))
    assert c_pow(full, full) == 0 and L.gft_series_last_form() == 2
    after()
    assert torch.equal(bits(big[:6 * 128].reshape(6, 2, 4, 16)), bits(series3.pow(f, 5)))
    assert torch.equal(bits(series3.compose(f, g, var=1)), bits(good))


# ---- streams ---------------------------------------------------------------------------------------------------------------------


def test_side_stream_is_ordered_with_torchs_work(oracle_lib):
    """pow's several launches and its pool workspace, and compose, behind a long kernel on a side stream: the result is consumed and
    the operand zeroed right after, with no host synchronisation"""
    from genfer_amd import series3

    B, n = 512, (2, 3, 4)
    x, g = dense((B,) + n, 41), small_g(n, 42, B)
    wp, wc = cc.want_pow(oracle_lib, x, 5, n), cc.want_compose(oracle_lib, x, g, 2, n)
    X, G = dev(x), dev(g)
    src = torch.zeros((B,) + n, dtype=torch.float64, device=DEV)
    series3.pow(src, 5), series3.compose(src, G, var=2)  # warm the kernels and the pool
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(20_000_000)  # the operand is produced behind a long kernel on this stream
        src.copy_(X)
        p = series3.pow(src, 5)
        c = series3.compose(src, G, var=2)
        twice = p * 2.0 + c  # consumed right after, no host synchronisation in between
        src.zero_()  # the operand is reused right after
    s.synchronize()
    assert_bits(p, wp, "pow on a side stream")
    assert_bits(c, wc, "compose on a side stream")
    assert_bits(twice, wp * 2.0 + wc, "consumer on the side stream")
