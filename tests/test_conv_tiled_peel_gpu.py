"""The peeled tiled product (gft_conv_tiled.hip conv_tiled_peel): a rank-3 product of full operands runs as the aligned
main part M (every tile's step range cut at the tile's first row, no masked lanes) plus the two leftover products L0 / L1
of the diagonal lane triangles, which add into z.  Forced with gft_set_option("tiled_peel", 1) on small shapes and
compared with the reference-order kernel (conv mode 1, itself bit-exact against the oracle): 1e-10 relative per
coefficient on positive data, the normwise bound against |x| (*) |y| on mixed signs."""
from math import lgamma, log

import numpy as np
import pytest

from conftest import splitmix64_uniform

pytestmark = pytest.mark.gpu


def rand(shape, seed, lo=0.0, hi=1.0):
    return (lo + (hi - lo) * splitmix64_uniform(seed, int(np.prod(shape)))).reshape(shape)


def conv(mode, x, y, zs, peel=1, slab=None, accumulate=False, z0=None):
    """gft_conv_raw on torch device buffers under conv mode `mode` and tiled_peel = `peel` (both restored)."""
    import torch

    import genfer_amd

    L = genfer_amd.lib()
    L.gft_set_conv_mode(mode)
    assert L.gft_set_option(b"tiled_peel", float(peel)) == 0
    try:
        tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        tz = torch.from_numpy(z0.copy()).cuda() if z0 is not None else torch.full(tuple(zs), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        lo, hi = (0, zs[0]) if slab is None else slab
        genfer_amd.conv_raw(tx.data_ptr(), x.shape, ty.data_ptr(), y.shape, tz.data_ptr(), zs, lo, hi, accumulate)
        L.gft_synchronize()
        return tz.cpu().numpy()
    finally:
        L.gft_set_option(b"tiled_peel", -1.0)
        L.gft_set_conv_mode(0)


def peeled():
    import genfer_amd

    return genfer_amd.op_stats()["tiled_peeled"]


# two tiles per axis (the smallest case with a leftover triangle and a batch axis); unequal lane axes with an inner length
# that is no multiple of 8; a batch of 8 = full 8x8 lane tiles on L0 and L1; the maximum inner length
PEEL_SHAPES = [(16, 16, 8), (24, 16, 20), (64, 64, 16), (16, 24, 128)]


@pytest.mark.parametrize("shape", PEEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_peeled_product_matches_reference_order_kernel(shape):
    x, y = rand(shape, 21), rand(shape, 22)
    want = conv(1, x, y, shape)
    n = peeled()
    got = conv(2, x, y, shape)
    assert peeled() == n + 1
    assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want)), np.abs((got - want) / want).max()
    assert got[0, 0, 0] == x[0, 0, 0] * y[0, 0, 0]
    # mixed signs: normwise against |x| (*) |y|
    xm, ym = 2 * x - 1, 2 * y - 1
    bound = conv(1, np.abs(xm), np.abs(ym), shape)
    assert np.all(np.abs(conv(2, xm, ym, shape) - conv(1, xm, ym, shape)) <= 1e-10 * bound)
    # deterministic (fixed launch order, fixed-order slab sums), and scaling by a power of two is exact
    assert np.array_equal(conv(2, x, y, shape), got)
    assert np.array_equal(conv(2, 2.0 * x, y, shape), 2.0 * got)
    # accumulate: M starts from the stored value, L0 and L1 add to it
    z0 = rand(shape, 23)
    acc = conv(2, x, y, shape, accumulate=True, z0=z0)
    assert np.all(np.abs(acc - (z0 + want)) <= 1e-10 * np.abs(z0 + want))
    assert peeled() == n + 5  # the five forced-tiled products above


@pytest.mark.parametrize("shape", PEEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_peeled_product_nonfinite_operands_fall_back(shape):
    """L0 and L1 carry the main part's guard: a product flagged non-finite is left, whole, to the reference-order kernel.
    Without `accumulate` that kernel overwrites z, whatever the tiled launches did to it; accumulating onto a finite z0
    shows that M, L0 and L1 left z alone (anything they added would be in the sum)."""
    x, y = rand(shape, 41), rand(shape, 42)
    xi, yi = x.copy(), y.copy()
    xi[3, 4, 5] = np.inf
    yi[9, 2, 3] = np.nan
    z0 = rand(shape, 43)
    for a, b in ((xi, y), (x, yi), (xi, yi)):
        n = peeled()
        got = conv(2, a, b, shape)
        assert peeled() == n + 1  # the peel was taken (and stood down on the device)
        assert np.array_equal(got, conv(1, a, b, shape), equal_nan=True)
        acc = conv(2, a, b, shape, accumulate=True, z0=z0)
        assert peeled() == n + 2
        assert np.array_equal(acc, conv(1, a, b, shape, accumulate=True, z0=z0), equal_nan=True)
    fin = conv(2, x, y, shape)  # the stamp is per product
    ref = conv(1, x, y, shape)
    assert np.all(np.isfinite(fin)) and np.all(np.abs(fin - ref) <= 1e-10 * np.abs(ref))


def test_peeled_product_pgf_like_dynamic_range():
    """Operands spanning more than 30 decades: relative accuracy per coefficient survives the split into three products."""
    n = 24
    shape = (n, n, n)
    i = np.arange(n)
    pois = lambda lam: np.exp(i * log(lam) - lam - np.array([lgamma(k + 1) for k in i]))
    pgf = pois(0.3)[:, None, None] * pois(20.0)[None, :, None] * pois(0.5)[None, None, :]
    x = pgf * (1 + 0.1 * rand(shape, 31))
    y = pgf[::-1, ::-1, ::-1].copy() * (1 + 0.1 * rand(shape, 32))
    assert x.max() / x.min() > 1e30 and x.min() > 0
    want = conv(1, x, y, shape)
    n0 = peeled()
    got = conv(2, x, y, shape)
    assert peeled() == n0 + 1
    assert want.min() > 0
    assert np.all(np.abs(got - want) <= 1e-10 * want), np.abs((got - want) / want).max()


def test_peel_is_not_taken_outside_its_structure():
    """Ragged / compact operands, rank 4 and slab-range calls keep the plain path even when the peel is forced."""
    n0 = peeled()
    xs, ys, zs = (20, 17, 29), (13, 22, 30), (30, 30, 40)
    x, y = rand(xs, 51), rand(ys, 52)
    want = conv(1, x, y, zs)
    assert np.all(np.abs(conv(2, x, y, zs) - want) <= 1e-10 * np.abs(want))
    r = (20, 17, 29)
    x, y = rand(r, 53), rand(r, 54)
    want = conv(1, x, y, r)
    assert np.all(np.abs(conv(2, x, y, r) - want) <= 1e-10 * np.abs(want))
    r4 = (16, 16, 16, 8)
    x, y = rand(r4, 55), rand(r4, 56)
    want = conv(1, x, y, r4)
    assert np.all(np.abs(conv(2, x, y, r4) - want) <= 1e-10 * np.abs(want))
    s = (16, 16, 8)
    x, y, z0 = rand(s, 57), rand(s, 58), rand(s, 59)
    want = conv(1, x, y, s)
    got = conv(2, x, y, s, slab=(4, 12), z0=z0)
    assert np.array_equal(got[:4], z0[:4]) and np.array_equal(got[12:], z0[12:])
    assert np.all(np.abs(got[4:12] - want[4:12]) <= 1e-10 * np.abs(want[4:12]))
    assert peeled() == n0
    conv(2, x, y, s, peel=0)  # switched off: the plain path, whatever the shape
    assert peeled() == n0


def test_peel_on_and_off_agree_at_64_cubed():
    """64^3 through auto conv mode, operands in the form auto mode peels at larger sizes: peel off, as auto decides (below
    its size threshold: not taken) and forced agree within 1e-10 — all three on the tiled kernel, only the forced one peeled."""
    import genfer_amd

    shape = (64, 64, 64)
    x, y = rand(shape, 61), rand(shape, 62)
    before = genfer_amd.op_stats()
    off = conv(0, x, y, shape, peel=0)
    after = genfer_amd.op_stats()
    assert after["tiled"] == before["tiled"] + 1 and after["tiled_peeled"] == before["tiled_peeled"]
    for peel, rise in ((-1, 0), (1, 1)):
        before = after
        on = conv(0, x, y, shape, peel=peel)
        after = genfer_amd.op_stats()
        assert after["tiled"] == before["tiled"] + 1 and after["tiled_peeled"] == before["tiled_peeled"] + rise
        assert np.all(np.abs(on - off) <= 1e-10 * np.abs(off)), np.abs((on - off) / off).max()


# Every instantiation family of the main kernel: full / compact / peel instantiation x NW = 1, 2, 4, 8 waves x the 8x8 lane
# tile (lane axes 16 x 16) / the run-time one (rank 2: 1 x 64).  NW follows from the result's inner length: 8 (16 where the
# operand must be compact: an x of inner length 8 spans the only chunk of a result of 8, so it is not compact there), 32,
# 64, 128 give 1, 2, 4, 8.  The peel exists on the 8x8 tile only.  Compared with the reference-order kernel as above.
def _dispatch_cases():
    for inner in (8, 32, 64, 128):
        for lanes, tile in (((16, 16), "8x8"), ((40,), "runtime")):
            yield pytest.param(lanes + (inner,), lanes + (inner,), 0, id=f"full-{tile}-{inner}")
            zi = max(inner, 16)
            yield pytest.param(lanes + (8,), lanes + (zi,), 0, id=f"compact-{tile}-{zi}")
        yield pytest.param((16, 16, inner), (16, 16, inner), 1, id=f"peel-8x8-{inner}")


@pytest.mark.parametrize("xs,zs,peel", list(_dispatch_cases()))
def test_tiled_dispatch_reaches_every_instantiation_family(xs, zs, peel):
    x, y = rand(xs, 71), rand(zs, 72)
    n = peeled()
    want = conv(1, x, y, zs, peel=peel)
    got = conv(2, x, y, zs, peel=peel)
    assert peeled() == n + peel
    assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want)), np.abs((got - want) / want).max()
    xm, ym = 2 * x - 1, 2 * y - 1  # mixed signs: normwise against |x| (*) |y|
    bound = conv(1, np.abs(xm), np.abs(ym), zs, peel=peel)
    assert np.all(np.abs(conv(2, xm, ym, zs, peel=peel) - conv(1, xm, ym, zs, peel=peel)) <= 1e-10 * bound)
