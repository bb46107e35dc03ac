"""The transposed bivariate product and the transposed Horner loop (genfer_amd.series2.corr / _compose_adj, gft_series2_corr /
gft_series2_compose_adj) on the MI355X.

corr is bit for bit the product of the flipped array -- flip(series2.mul(flip(g), y, n=g.shape))[..., :m0, :m1] -- at every size at
which the kernel takes another path (one wave, an odd number of outputs, more than one pass of the lanes, the limit), exact on small
integers against the numpy model of tests/_series2_adj_model.py, and the adjoint of mul; _compose_adj is bit for bit the unfused
loop of series2.corr calls at the compact shapes L_i, with g resident in LDS and with g read from global memory."""
import numpy as np
import pytest

import _series2_adj_model as A
from conftest import REL_TOL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield


def mixed(shape, seed):
    """mixed signs with some exact zeros"""
    rng = np.random.default_rng(seed)
    a = rng.random(shape) - 0.5
    a[rng.random(shape) < 0.15] = 0.0
    return a


def ints(shape, seed, lo=-3, hi=3):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int64)


def flip(t):
    return torch.flip(t, (-2, -1))


def corr(g, y, m=None, **kw):
    from genfer_amd import series, series2

    got = series2.corr(g, y, m, **kw)
    assert series.last_form() == "B"  # gft_series_last_form() == 2 after a series2 call
    return got


def by_flips(g, y, m=None):
    """the formulation corr replaces: flip, mul at g's shape, flip, slice"""
    from genfer_amd import series2

    m = tuple(g.shape[-2:]) if m is None else m
    return flip(series2.mul(flip(g), y, n=tuple(g.shape[-2:])))[..., :m[0], :m[1]]


def cases(g):
    """(y shape, m): y full and compact on each axis (ny0 = 1 and ny1 = 1 among them), m == g and m < g on each axis"""
    g0, g1 = g
    ys = {g, (1, g1), (g0, 1), (1, 1), (max(1, g0 // 2), g1), (g0, max(1, g1 // 2)), (max(1, g0 - 1), max(1, g1 - 1))}
    ms = {g, (max(1, g0 - 1), g1), (g0, max(1, g1 - 1)), (max(1, g0 // 2), max(1, g1 // 3)), (1, 1)}
    return [(y, m) for y in sorted(ys) for m in sorted(ms)]


# (8, 8): 64 coefficients, the last one-wave size; (9, 15): 135, odd, so the pairing has a middle output; (16, 33): the lanes take
# more than one pair each (264 pairs on 256 lanes)
@pytest.mark.parametrize("g", [(1, 1), (1, 7), (7, 1), (3, 5), (8, 8), (9, 15), (16, 33)])
def test_corr_is_the_flipped_product(g):
    B = 3
    for ys, m in cases(g):
        ga, ya = dev(mixed((B,) + g, 100 * g[0] + g[1])), dev(mixed((B,) + ys, 7 * ys[0] + ys[1]))
        got = corr(ga, ya, m)
        assert got.shape == (B,) + m
        assert torch.equal(bits(got), bits(by_flips(ga, ya, m))), (g, ys, m)
    # m defaults to g's stored shape
    assert torch.equal(bits(corr(ga, ya)), bits(by_flips(ga, ya)))


def test_corr_at_the_limit():
    """one item of (64, 64): 4096 coefficients, g and a full y are the whole 64 KB"""
    g, y = dev(mixed((1, 64, 64), 1)), dev(mixed((1, 64, 64), 2))
    assert torch.equal(bits(corr(g, y)), bits(by_flips(g, y)))
    ys = dev(mixed((33, 64), 3))
    assert torch.equal(bits(corr(g, ys, (64, 31))), bits(by_flips(g, ys, (64, 31))))


def test_corr_views():
    """a broadcast y with batch stride 0, operands that are row-strided slices of wider tensors, out= into a strided view, out is g"""
    B, g, ys, m = 3, (9, 15), (4, 15), (7, 11)
    ga, ya = dev(mixed((B,) + g, 11)), dev(mixed(ys, 12))
    want = by_flips(ga, ya.expand((B,) + ys).contiguous(), m)
    assert torch.equal(bits(corr(ga, ya, m)), bits(want))  # y: one item against the batch
    assert torch.equal(bits(corr(ga, ya.expand((B,) + ys), m)), bits(want))
    wide_g, wide_y = dev(mixed((B, 12, 40), 13)), dev(mixed((B, 6, 33), 14))
    gv, yv = wide_g[:, 2:11, 5:20], wide_y[:, 1:5, 3:18]  # row strides 40 and 33, offsets inside the rows
    assert gv.stride(-2) == 40 and yv.stride(-2) == 33
    want = by_flips(gv.contiguous(), yv.contiguous(), m)
    assert torch.equal(bits(corr(gv, yv, m)), bits(want))
    guard = float(np.float64(-7.25))
    buf = torch.full((B, 10, 30), guard, dtype=torch.float64, device=DEV)
    ov = buf[:, 1:8, 4:15]
    assert corr(gv, yv, m, out=ov) is ov
    assert torch.equal(bits(ov), bits(want))
    buf[:, 1:8, 4:15] = guard
    assert bool((buf == guard).all())  # nothing written outside the view
    # in place: the result is g itself (the same view), on a strided view too
    g2 = ga.clone()
    assert corr(g2, ya, out=g2) is g2
    assert torch.equal(bits(g2), bits(by_flips(ga, ya.expand((B,) + ys).contiguous())))
    w2 = wide_g.clone()
    v2 = w2[:, 2:11, 5:20]
    corr(v2, yv, out=v2)
    assert torch.equal(bits(v2), bits(by_flips(gv.contiguous(), yv.contiguous())))
    w2[:, 2:11, 5:20] = wide_g[:, 2:11, 5:20]
    assert torch.equal(bits(w2), bits(wide_g))
    # an empty batch is a no-op
    assert corr(ga[:0], ya, m).shape == (0,) + m


def test_corr_small_integers_against_the_model():
    B = 3
    for g, ys, m in [((3, 4), (3, 4), (3, 4)), ((3, 4), (2, 3), (2, 4)), ((5, 3), (1, 3), (5, 2)), ((4, 6), (4, 1), (3, 6)), ((9, 15), (4, 7), (9, 15))]:
        ga, ya = ints((B,) + g, g[0] + 10 * g[1]), ints((B,) + ys, ys[0] + 20 * ys[1])
        want = np.stack([A.corr2(ga[b], ya[b], m) for b in range(B)])
        assert np.array_equal(corr(dev(ga), dev(ya), m).cpu().numpy(), want), (g, ys, m)


@pytest.mark.parametrize("nx,ny,n", [((3, 5), (3, 5), (3, 5)), ((2, 3), (3, 5), (3, 5)), ((9, 15), (4, 15), (9, 15)), ((16, 20), (7, 33), (16, 33))])
def test_corr_is_the_adjoint_of_mul(nx, ny, n):
    """<mul(x, y, n), g> = <x, corr(g, y, x.shape)> within REL_TOL times the sum of absolute products"""
    from genfer_amd import series2

    B = 3
    x, y, g = dev(mixed((B,) + nx, 31)), dev(mixed((B,) + ny, 32)), dev(mixed((B,) + n, 33))
    z, c = series2.mul(x, y, n), corr(g, y, nx)
    lhs, rhs = (z * g).sum((-2, -1)), (x * c).sum((-2, -1))
    scale = (series2.mul(x.abs(), y.abs(), n) * g.abs()).sum((-2, -1))
    print(f"adjoint identity {nx} {ny} {n}: worst {float(((lhs - rhs).abs() / scale).max()):.3e} of the sum of absolute products")
    assert bool(((lhs - rhs).abs() <= REL_TOL * scale).all())


# ---- the transposed Horner loop ------------------------------------------------------------------------------------------------------


def adj(gh, g, var, nf, **kw):
    from genfer_amd import series, series2

    got = series2._compose_adj(gh, g, var, nf, **kw)
    assert series.last_form() == "B"
    return got


def unfused(gh, g, var, nf):
    """the loop of series2.corr calls at the compact shapes L_i (tests/_series2_adj_model.py with the device's corr)"""
    from genfer_amd import series2

    B = torch.broadcast_shapes(gh.shape[:-2], g.shape[:-2])
    return A.compose_adj(gh.expand(B + gh.shape[-2:]), g, var, nf, corr=lambda a, y, m: series2.corr(a.contiguous(), y, m))


ADJ_CASES = [  # f, g, n: 1, 2 and 5 slices for either var among them
    ((5, 3), (2, 3), (6, 7)),  # one axis saturates at n before the other
    ((3, 5), (3, 2), (7, 6)),
    ((1, 4), (2, 3), (3, 4)), ((4, 1), (2, 3), (4, 3)),  # a single slice (var 0 resp. var 1)
    ((2, 4), (3, 3), (4, 5)), ((4, 2), (3, 3), (5, 4)),  # two slices
    ((4, 3), (1, 3), (5, 6)), ((3, 4), (3, 1), (6, 5)),  # ng == 1 on the substituted axis (var 0 resp. var 1) and on the other one
    ((5, 5), (9, 15), (9, 15)),  # more than one wave
]


@pytest.mark.parametrize("var", [0, 1])
@pytest.mark.parametrize("f,g,n", ADJ_CASES)
def test_compose_adj_is_the_unfused_loop(f, g, n, var):
    B = 3
    gh, ga = dev(mixed((B,) + n, 50 * n[0] + n[1] + var)), dev(mixed((B,) + g, 60 * g[0] + g[1] + var))
    got = adj(gh, ga, var, f)
    assert got.shape == (B,) + f
    assert torch.equal(bits(got), bits(unfused(gh, ga, var, f))), (f, g, n, var)
    one = dev(mixed(g, 9))  # a broadcast g: one item against the batch
    assert torch.equal(bits(adj(gh, one, var, f)), bits(unfused(gh, one.expand((B,) + g).contiguous(), var, f)))


def test_compose_adj_with_one_slice_does_not_read_g():
    gh, g = dev(mixed((3, 3, 4), 1)), torch.full((3, 2, 2), float("nan"), dtype=torch.float64, device=DEV)
    assert torch.equal(bits(adj(gh, g, 0, (1, 4))), bits(gh[:, :1, :4]))
    assert torch.equal(bits(adj(gh, g, 1, (3, 1))), bits(gh[:, :3, :1]))


def test_compose_adj_with_g_in_global_memory():
    """one item of n = (64, 64), g = (64, 33), f = (3, 64), var 0: two arrays of 64 KB and g's 16.5 KB exceed every grant"""
    gh, g = dev(mixed((1, 64, 64), 4)), dev(mixed((1, 64, 33), 5))
    assert torch.equal(bits(adj(gh, g, 0, (3, 64))), bits(unfused(gh, g, 0, (3, 64))))


def test_compose_adj_small_integers_and_views():
    B, f, g, n = 3, (3, 4), (2, 3), (5, 6)
    for var in (0, 1):
        gha, ga = ints((B,) + n, 3 + var), ints((B,) + g, 5 + var)
        want = np.stack([A.compose_adj(gha[b], ga[b], var, f) for b in range(B)])
        assert np.array_equal(adj(dev(gha), dev(ga), var, f).cpu().numpy(), want), var
        wide = dev(ints((B, 8, 11), 7))
        wide[:, 2:7, 3:9] = dev(gha)
        buf = torch.full((B, 5, 9), -7.25, dtype=torch.float64, device=DEV)
        ov = buf[:, 1:4, 2:6]
        assert adj(wide[:, 2:7, 3:9], dev(ga), var, f, out=ov) is ov  # a row-strided gh, out= into a strided view
        assert np.array_equal(ov.cpu().numpy(), want)
        buf[:, 1:4, 2:6] = -7.25
        assert bool((buf == -7.25).all())


# ---- aliasing ---------------------------------------------------------------------------------------------------------------------


def test_partial_overlap_is_refused():
    from genfer_amd import series2
    from genfer_amd.taylor import TaylorError

    buf = dev(mixed((3, 8, 8), 1))
    g, y = buf[:, :6, :6], dev(mixed((3, 2, 2), 2))
    with pytest.raises(TaylorError, match="partially overlaps g"):
        series2.corr(g, y, out=buf[:, 1:7, 1:7])  # a shifted window of the same buffer
    with pytest.raises(TaylorError, match="partially overlaps g"):
        series2.corr(g, y, (5, 6), out=buf[:, :5, :6])  # the leading rows of g: not the same view
    small = buf[:, :2, :2]
    with pytest.raises(TaylorError, match="partially overlaps y"):
        series2.corr(dev(mixed((3, 2, 2), 3)), small, out=small)  # the result is never y
    with pytest.raises(TaylorError, match="partially overlaps g"):
        series2._compose_adj(dev(mixed((3, 2, 2), 4)), small, 0, (2, 2), out=small)  # nor compose_adj's g
    with pytest.raises(TaylorError, match="partially overlaps gh"):
        series2._compose_adj(g, y, 0, (2, 6), out=buf[:, 1:3, :6])
    before = buf.clone()
    gh = buf[:, :6, :6]
    want = unfused(gh.contiguous(), y, 1, (6, 6))
    series2._compose_adj(gh, y, 1, (6, 6), out=gh)  # the result may be gh itself (the same view)
    assert torch.equal(bits(gh), bits(want))
    assert torch.equal(bits(buf[:, 6:, :]), bits(before[:, 6:, :])) and torch.equal(bits(buf[:, :, 6:]), bits(before[:, :, 6:]))
