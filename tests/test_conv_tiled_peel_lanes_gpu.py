"""The two lanes of a peeled tiled product (gft_conv_tiled.hip conv_tiled_peel, option "tiled_peel_lanes"): the main
kernels of the leftover products L0 and L1 are issued on the library's two internal streams beside the aligned main part
M, each with partial slabs of its own (gft_peel_layout.hpp), and joined before L0's reduce.  z is written in the same order
as on one stream, so the option must not change a bit; nothing may outrun the join; the non-finite guard stands all three
launches down wherever they run.

Peel forced with "tiled_peel" = 1 on small shapes, grids capped with "tiled_slots" (a cap below the number of ranges takes
the claiming path).  Reference: the reference-order kernel (conv mode 1).  Bar: 1e-10 relative per coefficient on positive
splitmix data, as the peel's own test uses: a coefficient is a sum of at most 64 * 64 * 16 = 16 * 24 * 128 < 65536 products,
so two orders of summation differ by at most 2 (n + 1) u = 1.5e-11 of the coefficient (u = 2^-53)."""
import numpy as np
import pytest

from conftest import splitmix64_uniform

pytestmark = pytest.mark.gpu

CAPS = (1, 3, 8, 0)
# the smallest peel there is; uneven lane axes; the longest inner axis; more ranges than a capped grid
SHAPES = [(16, 16, 8), (24, 16, 20), (16, 24, 128), (64, 64, 16)]


def rand(shape, seed, lo=0.0, hi=1.0):
    return (lo + (hi - lo) * splitmix64_uniform(seed, int(np.prod(shape)))).reshape(shape)


class knobs:
    """conv mode, tiled_peel, tiled_slots and tiled_peel_lanes for the calls inside, all restored."""

    def __init__(self, mode, peel=1, cap=0, lanes=1):
        self.mode, self.peel, self.cap, self.lanes = mode, peel, cap, lanes

    def __enter__(self):
        import genfer_amd

        L = self.L = genfer_amd.lib()
        L.gft_set_conv_mode(self.mode)
        assert L.gft_set_option(b"tiled_peel", float(self.peel)) == 0
        assert L.gft_set_option(b"tiled_slots", float(self.cap)) == 0
        assert L.gft_set_option(b"tiled_peel_lanes", float(self.lanes)) == 0
        return L

    def __exit__(self, *exc):
        self.L.gft_set_option(b"tiled_peel_lanes", -1.0)
        self.L.gft_set_option(b"tiled_slots", 0.0)
        self.L.gft_set_option(b"tiled_peel", -1.0)
        self.L.gft_set_conv_mode(0)


def upload(*arrays):
    import torch

    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return t


def outputs(*specs):
    """Result tensors, one per spec: a shape (NaN-filled) or an array to accumulate onto; allocated and synchronised."""
    import torch

    t = [torch.from_numpy(z.copy()).cuda() if isinstance(z, np.ndarray) else torch.full(tuple(z), np.nan, dtype=torch.float64, device="cuda")
         for z in specs]
    torch.cuda.synchronize()
    return t


def issue(tx, ty, tz, accumulate=False):
    """One gft_conv_raw on device tensors: no allocation, no synchronisation."""
    import genfer_amd

    zs = tuple(tz.shape)
    genfer_amd.conv_raw(tx.data_ptr(), tuple(tx.shape), ty.data_ptr(), tuple(ty.shape), tz.data_ptr(), zs, 0, zs[0], accumulate)
    return tz


def conv(mode, x, y, zs, peel=1, cap=0, lanes=1, accumulate=False, z0=None):
    """The product alone: synchronised before and after."""
    tx, ty = upload(x, y)
    (tz,) = outputs(z0 if accumulate else zs)
    with knobs(mode, peel, cap, lanes) as L:
        issue(tx, ty, tz, accumulate)
        L.gft_synchronize()
        return tz.cpu().numpy()


def stats():
    import genfer_amd

    s = genfer_amd.op_stats()
    return {k: s[k] for k in ("tiled_peel_forked", "tiled_peeled", "launches")}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lanes_do_not_change_a_bit(shape):
    x, y, z0 = rand(shape, 11), rand(shape, 12), rand(shape, 13)
    for kw in (dict(), dict(accumulate=True, z0=z0)):
        want = conv(1, x, y, shape, **kw)
        got, rise = {}, {}
        for lanes in (0, 1):
            for cap in CAPS:
                before = stats()
                got[lanes, cap] = conv(2, x, y, shape, cap=cap, lanes=lanes, **kw)
                after = stats()
                rise[lanes, cap] = {k: after[k] - before[k] for k in after}
        first = got[0, CAPS[0]]
        assert np.all(np.isfinite(first))
        err = np.abs(first - want) / np.abs(want)
        print(f"{shape} accumulate {bool(kw)}: max relative error {err.max():.3e}")
        assert np.all(np.abs(first - want) <= 1e-10 * np.abs(want)), err.max()
        for key, g in got.items():
            assert np.array_equal(g, first), key
        for cap in CAPS:
            off, on = rise[0, cap], rise[1, cap]
            assert off["tiled_peeled"] == 1 and on["tiled_peeled"] == 1, cap
            assert off["tiled_peel_forked"] == 0 and on["tiled_peel_forked"] == 1, cap
            assert on["launches"] == off["launches"], cap


def _chain_on(stream):
    """A (peeled, lanes on), B (plain, small: its counters and slabs lie over the first bytes of the workspace), A again into
    a second output, then a read of all three: on `stream`, a caller's, by a consumer queued behind them there; None: on the
    library's own, after gft_synchronize.  Nothing is synchronised in between.  A is 16 x 16 x 128 under a cap of one
    workgroup per launch: its leftover launches have seven times the steps of its main part (672 against 100, of 136 chunk
    products each), so a reduce that did not wait for the lanes would read slabs that are still being written."""
    import torch

    import genfer_amd

    a, b = (16, 16, 128), (32, 32, 64)
    xa, ya, xb, yb = rand(a, 21), rand(a, 22), rand(b, 23), rand(b, 24)
    alone_a = conv(2, xa, ya, a, peel=1, cap=1, lanes=1)
    alone_b = conv(2, xb, yb, b, peel=0, cap=1, lanes=1)
    txa, tya, txb, tyb = upload(xa, ya, xb, yb)
    r1, r2, r3 = outputs(a, b, a)
    L = genfer_amd.lib()
    with knobs(2, peel=1, cap=1, lanes=1):
        before = stats()
        if stream is None:
            issue(txa, tya, r1)
            L.gft_set_option(b"tiled_peel", 0.0)
            issue(txb, tyb, r2)
            L.gft_set_option(b"tiled_peel", 1.0)
            issue(txa, tya, r3)
            L.gft_synchronize()
            out = [r.cpu().numpy() for r in (r1, r2, r3)]
        else:
            assert L.gft_set_stream(stream.cuda_stream) == 0
            try:
                with torch.cuda.stream(stream):
                    issue(txa, tya, r1)
                    L.gft_set_option(b"tiled_peel", 0.0)
                    issue(txb, tyb, r2)
                    L.gft_set_option(b"tiled_peel", 1.0)
                    issue(txa, tya, r3)
                    copies = [r.clone() for r in (r1, r2, r3)]  # the consumer: queued on the caller's stream, behind the library's launches
                stream.synchronize()
                out = [c.cpu().numpy() for c in copies]
            finally:
                assert L.gft_set_stream(None) == 0
        assert stats()["tiled_peel_forked"] == before["tiled_peel_forked"] + 2
    assert np.array_equal(out[0], alone_a) and np.array_equal(out[2], alone_a)
    assert np.array_equal(out[1], alone_b)
    want_a = conv(1, xa, ya, a)
    assert np.all(np.abs(alone_a - want_a) <= 1e-10 * np.abs(want_a))


def test_nothing_outruns_the_join():
    _chain_on(None)


def test_nothing_outruns_the_join_on_a_callers_stream():
    import torch

    _chain_on(torch.cuda.Stream())


@pytest.mark.parametrize("shape", [(24, 16, 20)], ids=["24x16x20"])
def test_guard_stands_the_lanes_down(shape):
    """One inf in x, one NaN in y, lanes on: M on the product's stream and L0, L1 on the lanes all return before they claim
    anything, the guarded reference-order launch owns z — accumulating onto a finite z0 gives its bits, non-finite pattern
    included (anything a tiled launch added would be in the sum) — and a finite product issued right behind, unsynchronised,
    claims from counters that read zero."""
    x, y = rand(shape, 31), rand(shape, 32)
    xi, yn = x.copy(), y.copy()
    xi[3, 4, 5] = np.inf
    yn[9, 2, 3] = np.nan
    z0 = rand(shape, 33)
    want_fin = conv(1, x, y, shape)
    for a, b in ((xi, y), (x, yn)):
        want_bad = conv(1, a, b, shape, accumulate=True, z0=z0)
        ta, tb, tx, ty = upload(a, b, x, y)
        r1, r2 = outputs(z0, shape)
        with knobs(2, peel=1, cap=3, lanes=1) as L:
            before = stats()
            issue(ta, tb, r1, accumulate=True)
            issue(tx, ty, r2)
            L.gft_synchronize()
            assert stats()["tiled_peel_forked"] == before["tiled_peel_forked"] + 2
            got_bad, got_fin = r1.cpu().numpy(), r2.cpu().numpy()
        assert not np.all(np.isfinite(got_bad))
        assert np.array_equal(got_bad, want_bad, equal_nan=True)
        assert np.all(np.isfinite(got_fin)) and np.all(np.abs(got_fin - want_fin) <= 1e-10 * np.abs(want_fin))
        assert np.array_equal(got_fin, conv(2, x, y, shape, cap=0, lanes=0))
