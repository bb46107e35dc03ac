"""The persistent launch of the tiled product (gft_conv_tiled.hip claim_range, launch_grid): a plan with more stream-K ranges
than the launch has workgroups is run by workgroups that CLAIM ranges from ticket counters at the front of the workspace.
gft_set_option("tiled_slots", n) caps the launched grid at n workgroups and never changes the cuts, so under a cap below
the number of ranges any shape takes the claiming path, and the result must not depend on the cap: every range is run
exactly once (z is pre-filled with NaN: a missed range leaves NaN or a short sum, a range run twice breaks the bar), by
whichever workgroup (the partial slabs are summed in plan order: bit-identical results).  With a cap below 8 some of the
eight queues have no workgroup of their own and are emptied by the others.

Reference: the reference-order kernel (conv mode 1, itself bit-exact against the oracle).  Bar: 1e-10 relative per
coefficient on positive splitmix data, the normwise bound against |x| (*) |y| on mixed signs.  The reference
alone stays inside that bar on these inputs whatever the summation order: a coefficient is a sum of at most
64 * 64 * 16 = 32 * 32 * 64 = 65536 products (144 * 144 * 8 = 165888 for the largest case), so two orders of summation differ
by at most 2 (n + 1) u = 3.7e-11 of sum |x||y| (u = 2^-53), which on positive data is the coefficient itself."""
import numpy as np
import pytest

from conftest import splitmix64_uniform

pytestmark = pytest.mark.gpu

CAPS = (1, 3, 8, 0)


def rand(shape, seed, lo=0.0, hi=1.0):
    return (lo + (hi - lo) * splitmix64_uniform(seed, int(np.prod(shape)))).reshape(shape)


class knobs:
    """conv mode, tiled_peel and tiled_slots for the calls inside, all restored."""

    def __init__(self, mode, peel=0, cap=0):
        self.mode, self.peel, self.cap = mode, peel, cap

    def __enter__(self):
        import genfer_amd

        L = self.L = genfer_amd.lib()
        L.gft_set_conv_mode(self.mode)
        assert L.gft_set_option(b"tiled_peel", float(self.peel)) == 0
        assert L.gft_set_option(b"tiled_slots", float(self.cap)) == 0
        return L

    def __exit__(self, *exc):
        self.L.gft_set_option(b"tiled_slots", 0.0)
        self.L.gft_set_option(b"tiled_peel", -1.0)
        self.L.gft_set_conv_mode(0)


def issue(x, y, zs, slab=None, accumulate=False, z0=None):
    """One gft_conv_raw on torch device buffers, NOT synchronised; returns the result tensor (NaN-filled unless z0)."""
    import torch

    import genfer_amd

    tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    tz = torch.from_numpy(z0.copy()).cuda() if z0 is not None else torch.full(tuple(zs), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lo, hi = (0, zs[0]) if slab is None else slab
    genfer_amd.conv_raw(tx.data_ptr(), x.shape, ty.data_ptr(), y.shape, tz.data_ptr(), zs, lo, hi, accumulate)
    return tx, ty, tz


def conv(mode, x, y, zs, peel=0, cap=0, **kw):
    with knobs(mode, peel, cap) as L:
        tz = issue(x, y, zs, **kw)[2]
        L.gft_synchronize()
        return tz.cpu().numpy()


# (xs, ys, zs, peel, slab, accumulate)
CASES = {
    "32x32x64": ((32, 32, 64),) * 3 + (0, None, False),          # 1024 ranges of about 6 steps
    "16x16x8-peel": ((16, 16, 8),) * 3 + (1, None, False),        # M, L0 and L1 all claim
    "64x64x16-peel": ((64, 64, 16),) * 3 + (1, None, False),
    "rank4-6x16x16x16": ((6, 16, 16, 16),) * 3 + (0, None, False),
    "rank2-64x100": ((64, 100),) * 3 + (0, None, False),          # the 1 x 64 lane tile
    "ragged": ((20, 17, 29), (13, 22, 30), (30, 30, 40), 0, None, False),
    "slab-5-19-of-24x16x40": ((24, 16, 40),) * 3 + (0, (5, 19), False),
    "accumulate-24x16x20-peel": ((24, 16, 20),) * 3 + (1, None, True),
    # the smallest cube-like shape whose plan has more ranges than the device has slots (8192 ranges on 4096 one-wave
    # slots at 256 CUs): cap 0 is the persistent launch a large product gets by default, with tapered ranges
    "144x144x8": ((144, 144, 8),) * 3 + (0, None, False),
}


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_result_does_not_depend_on_who_runs_a_range(case):
    xs, ys, zs, peel, slab, accumulate = CASES[case]
    x, y = rand(xs, 81), rand(ys, 82)
    z0 = rand(zs, 83) if accumulate or slab else None
    kw = dict(slab=slab, accumulate=accumulate, z0=z0)
    rows = slice(*slab) if slab else slice(None)
    for xm, ym, positive in ((x, y, True), (2 * x - 1, 2 * y - 1, False)):
        want = conv(1, xm, ym, zs, **kw)
        bound = np.abs(want) if positive and not accumulate else conv(1, np.abs(xm), np.abs(ym), zs, **kw)
        got = [conv(2, xm, ym, zs, peel=peel, cap=cap, **kw) for cap in CAPS]
        for cap, g in zip(CAPS, got):
            assert np.all(np.isfinite(g)), cap
            err = np.abs(g - want)[rows] / bound[rows]
            print(f"{case} cap {cap} positive {positive}: max error / bound {err.max():.3e}")
            assert np.all(np.abs(g - want)[rows] <= 1e-10 * bound[rows]), (cap, err.max())
            assert np.array_equal(g, got[0]), cap
        if slab:  # the rows outside the slab range are the caller's
            assert np.array_equal(got[0][: slab[0]], z0[: slab[0]]) and np.array_equal(got[0][slab[1]:], z0[slab[1]:])


def test_counters_are_zero_again_for_the_next_product():
    """A, B of another shape, and A again under cap 3 with no synchronisation between them: every call's counters start
    from zero in stream order, whatever the call before left in the workspace (B's partial slabs lie over A's counters'
    neighbours, the peeled A has three counter sets)."""
    a, b = (64, 64, 16), (32, 32, 64)
    xa, ya, xb, yb = rand(a, 91), rand(a, 92), rand(b, 93), rand(b, 94)
    want_a, want_b = conv(1, xa, ya, a), conv(1, xb, yb, b)
    with knobs(2, peel=1, cap=3) as L:
        r1 = issue(xa, ya, a)
        r2 = issue(xb, yb, b)
        r3 = issue(xa, ya, a)
        L.gft_synchronize()
        a1, b1, a2 = (r[2].cpu().numpy() for r in (r1, r2, r3))
    assert np.all(np.abs(a1 - want_a) <= 1e-10 * np.abs(want_a))
    assert np.all(np.abs(b1 - want_b) <= 1e-10 * np.abs(want_b))
    assert np.array_equal(a1, a2)
    assert np.array_equal(a1, conv(2, xa, ya, a, peel=1, cap=0)) and np.array_equal(b1, conv(2, xb, yb, b, peel=1, cap=0))


@pytest.mark.parametrize("shape,peel", [((24, 16, 20), 1), ((32, 32, 64), 0)], ids=["24x16x20-peel", "32x32x64"])
def test_guard_stands_claiming_launches_down(shape, peel):
    """An operand holding inf: every workgroup returns before it claims anything, the counters stay as the memset left them,
    and the guarded reference-order launch owns z — accumulating onto a finite z0 gives the reference-order result bit for
    bit (anything a tiled launch added would be in the sum).  A finite product issued right behind it, unsynchronised,
    claims from zeroed counters and is correct."""
    x, y = rand(shape, 95), rand(shape, 96)
    xi = x.copy()
    xi[3, 4, 5] = np.inf
    z0 = rand(shape, 97)
    want_inf = conv(1, xi, y, shape, accumulate=True, z0=z0)
    want_fin = conv(1, x, y, shape)
    with knobs(2, peel=peel, cap=3) as L:
        r1 = issue(xi, y, shape, accumulate=True, z0=z0)
        r2 = issue(x, y, shape)
        L.gft_synchronize()
        got_inf, got_fin = r1[2].cpu().numpy(), r2[2].cpu().numpy()
    assert np.array_equal(got_inf, want_inf, equal_nan=True)
    assert np.all(np.isfinite(got_fin)) and np.all(np.abs(got_fin - want_fin) <= 1e-10 * np.abs(want_fin))
