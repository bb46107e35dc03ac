"""Device interop on the MI355X: TaylorPoly.from_torch / to_torch (gft_from_device / gft_to_device and their gfti_ twins).

Bits in, bits out (every view torch makes, every handle state), the same results as handles built from host data, the stream
contract with torch's streams (no host stall, safe reuse of the caller's memory) and the refusals."""
import ctypes

import numpy as np
import pytest

from conftest import splitmix64_uniform

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)


def _cls(W):
    import genfer_amd

    return genfer_amd.TaylorPoly if W == 1 else genfer_amd.IntervalTaylorPoly


def _default_host_tier():
    import genfer_amd

    assert genfer_amd.lib().gft_set_option(b"host_max_elems", -1.0) == 0


def bits(t):
    return t.contiguous().view(torch.int64)


SPECIALS = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,  # +-0, +-inf
                     0x7FF8000000000123, 0xFFF4000000000ABC, 0x7FF0000000000001,  # NaNs with payloads (one signalling)
                     0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x0008000000000000],  # subnormals
                    dtype=np.uint64).view(np.int64)


def rand_bits(shape, seed):
    """Random 64-bit patterns (every class of double, NaN payloads included), the specials first."""
    n = int(np.prod(shape)) if len(shape) else 1
    g = torch.Generator(device="cpu").manual_seed(seed)
    v = torch.randint(-(2**63), 2**63 - 1, (n,), dtype=torch.int64, generator=g)
    k = min(n, len(SPECIALS))
    v[:k] = torch.from_numpy(SPECIALS[:k])
    return v.view(torch.float64).reshape(shape).to(DEV)


def views(full, seed):
    """(name, tensor of shape `full`) for the layouts torch hands out."""
    yield "contiguous", rand_bits(full, seed)
    if len(full) == 0:
        return
    last = full[-1]
    yield "step2", rand_bits(full[:-1] + (2 * last,), seed + 1)[..., ::2]
    yield "narrowed", rand_bits(full[:-1] + (last + 3,), seed + 2)[..., :last]
    if len(full) >= 2:
        rev = tuple(reversed(range(len(full))))
        yield "permuted", rand_bits(tuple(full[p] for p in rev), seed + 3).permute(*rev)
        yield "plane_last", rand_bits(full[1:] + full[:1], seed + 4).movedim(-1, 0)
    if len(full) == 2:
        yield "t", rand_bits((full[1], full[0]), seed + 5).t()
    yield "expanded", rand_bits((1,) + full[1:], seed + 6).expand(*full)


ROUND_TRIP_SHAPES = [(), (1,), (7,), (3, 5), (40, 70), (4, 6, 5), (20, 33, 17), (2, 3, 4, 5), (9, 8, 7, 6), (2, 3, 2, 3, 4),
                     (5, 4, 6, 3, 7)]


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("shape", ROUND_TRIP_SHAPES, ids=lambda s: "x".join(map(str, s)) or "scalar")
def test_round_trip_is_bit_identical(W, shape):
    _default_host_tier()  # (from_torch ignores the host tier whatever the threshold: sizes on both sides of it are here)
    TP = _cls(W)
    full = ((2,) + shape) if W == 2 else shape
    for name, v in views(full, seed=len(shape) * 10 + W):
        p = TP.from_torch(v)
        assert p.coeffs_shape() == shape and p.degrees_p1() == shape
        got = p.to_torch()
        assert got.shape == v.shape and got.is_contiguous()
        assert torch.equal(bits(got), bits(v)), name
        assert np.array_equal(p.array().view(np.int64), bits(v).cpu().numpy()), name
        if len(full) >= 2:  # into a transposed `out`
            rev = tuple(reversed(range(len(full))))
            out = torch.empty(tuple(full[q] for q in rev), dtype=torch.float64, device=DEV).permute(*rev)
            assert p.to_torch(out=out) is out
            assert torch.equal(bits(out), bits(v)), name
        if len(full) >= 1:  # into a strided slice of a larger `out`; the rest untouched
            big = torch.full(full[:-1] + (2 * full[-1] + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV).view(torch.float64)
            p.to_torch(out=big[..., 1::2])
            assert torch.equal(bits(big[..., 1::2]), bits(v)), name
            assert bool((big[..., 0::2].contiguous().view(torch.int64) == 0x5A5A5A5A5A5A5A5A).all()), name


# ---- same values, same bits as handles built from host data -----------------------------------------------------------------


def values(shape, seed, lo=0.5, hi=1.5, W=1):
    n = int(np.prod(shape))
    a = (lo + (hi - lo) * splitmix64_uniform(seed, n)).reshape(shape)
    if W == 2:
        a = np.stack([a, a + 1e-3 * splitmix64_uniform(seed + 99, n).reshape(shape)])
    return a


def pair(TP, arr, deg=None):
    """The same coefficients as a handle from host data (new) and from a device tensor (from_torch)."""
    shape = arr.shape[1:] if TP.WIDTH == 2 else arr.shape
    deg = tuple(shape) if deg is None else tuple(deg)
    return TP.new(arr, deg), TP.from_torch(torch.from_numpy(arr).to(DEV), deg)


def same_bits(h, d):
    assert h.coeffs_shape() == d.coeffs_shape() and h.degrees_p1() == d.degrees_p1()
    a, b = h.array(), d.array()
    assert np.array_equal(a.view(np.int64), b.view(np.int64)), np.max(np.abs(a - b))


@pytest.mark.parametrize("W", [1, 2])
def test_operations_match_host_built_handles(W):
    TP = _cls(W)
    # a 64^3-class general product
    xh, xd = pair(TP, values((32, 32, 32), 1, W=W), (64, 64, 64))
    yh, yd = pair(TP, values((32, 32, 32), 2, W=W), (64, 64, 64))
    same_bits(xh * yh, xd * yd)
    # an n == 2 affine operand (from_host keeps it as host values; from_device has a device tensor)
    ah, ad = pair(TP, values((6, 5), 3, W=W))
    bh, bd = pair(TP, values((1, 2), 4, W=W), (6, 5))
    same_bits(ah * bh, ad * bd)
    # recurrences, substitution, axis sums
    ph, pd = pair(TP, values((12, 10), 5, W=W))
    qh, qd = pair(TP, values((12, 10), 6, W=W))
    same_bits(ph / qh, pd / qd)
    same_bits(ph.exp(), pd.exp())
    same_bits(ph.log(), pd.log())
    sh, sd = pair(TP, values((12, 10), 7, lo=0.0, hi=0.5, W=W))
    same_bits(ph.subst_var(0, sh), pd.subst_var(0, sd))
    same_bits(ph.shift_down(1, 2), pd.shift_down(1, 2))

    # adds and scalings the deferred launch graph records
    def chain(p, q):
        r = p * TP.from_scalar(2.5) + q * TP.from_scalar(-0.75)
        return (r - p * TP.from_scalar(0.5)) * TP.from_scalar(3.0) + q

    same_bits(chain(ph, qh), chain(pd, qd))


def test_product_matches_oracle(OTP):
    import genfer_amd

    x, y = values((20, 18, 16), 11), values((20, 18, 16), 12)
    deg = (30, 30, 30)
    got = (genfer_amd.TaylorPoly.from_torch(torch.from_numpy(x).to(DEV), deg) *
           genfer_amd.TaylorPoly.from_torch(torch.from_numpy(y).to(DEV), deg)).to_torch().cpu().numpy()
    want = (OTP.new(x, deg) * OTP.new(y, deg)).array()
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want))


# ---- export materialises every handle state -------------------------------------------------------------------------------


@pytest.mark.parametrize("W", [1, 2])
def test_export_materialises_every_handle_state(W):
    import genfer_amd

    TP = _cls(W)
    sc = (1.25, 1.5) if W == 2 else 1.25

    def check(make, first_export=True):
        p = make()
        if first_export:  # to_torch is the first consumer of the values
            got = p.to_torch().cpu().numpy()
            want = make().array()
        else:
            want = p.array()
            got = p.to_torch().cpu().numpy()
        assert np.array_equal(got.view(np.int64), want.view(np.int64))

    check(lambda: TP.from_scalar(sc))  # lazy scalar
    check(lambda: TP.var(1, sc, 5))  # lazy affine value
    _default_host_tier()
    small = values((6, 7), 21, W=W)
    st0 = genfer_amd.op_stats()["host_tier_ops"]
    check(lambda: TP.new(small, (6, 7)) * TP.new(small, (6, 7)))  # host-tier result
    assert genfer_amd.op_stats()["host_tier_ops"] > st0
    assert genfer_amd.lib().gft_set_option(b"host_max_elems", 0.0) == 0
    big = values((50, 60), 22, W=W)
    d0 = genfer_amd.op_stats()["deferred_ops"]
    check(lambda: TP.new(big, (50, 60)) * TP.from_scalar(sc))  # deferred chain
    assert genfer_amd.op_stats()["deferred_ops"] > d0
    other = values((50, 60), 23, W=W)
    g0 = genfer_amd.op_stats()["graph_recordings"]
    rec = lambda: TP.new(big, (50, 60)) * TP.from_scalar(sc) + TP.new(other, (50, 60)) * TP.from_scalar(0.5)  # noqa: E731
    check(rec)  # graph recording (GFT_BATCH on, the default)
    check(rec, first_export=False)
    assert genfer_amd.op_stats()["graph_recordings"] > g0


# ---- stream contract --------------------------------------------------------------------------------------------------------


def _sleep_cycles_for_ms(ms):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(1_000_000)
    b.record()
    b.synchronize()
    per_ms = 1_000_000 / max(a.elapsed_time(b), 1e-3)
    return int(min(per_ms * ms, 2**40))


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("which", ["side_stream", "null_stream"])
def test_import_is_stream_ordered_without_host_stall(W, which):
    TP = _cls(W)
    full = (W, 64, 48) if W == 2 else (64, 48)
    src = torch.zeros(full, dtype=torch.float64, device=DEV)
    warm = TP.from_torch(src)  # warm the pool block and the kernel
    del warm
    cycles = _sleep_cycles_for_ms(100)
    s = torch.cuda.Stream() if which == "side_stream" else torch.cuda.default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert (torch.cuda.current_stream().cuda_stream == 0) == (which == "null_stream")
        torch.cuda._sleep(cycles)
        src.fill_(7.5)
        p = TP.from_torch(src)
        assert not s.query(), "from_torch waited for the caller's stream on the host"
    s.synchronize()
    assert np.all(p.array() == 7.5)


@pytest.mark.parametrize("W", [1, 2])
def test_source_and_destination_reuse_is_safe(W):
    TP = _cls(W)
    full = (W, 96, 80) if W == 2 else (96, 80)
    cycles = _sleep_cycles_for_ms(20)
    src = rand_bits(full, 31)
    want = src.clone()
    torch.cuda._sleep(cycles)  # the caller's stream is busy when the import is issued
    p = TP.from_torch(src)
    del src
    junk = [torch.full(full, 99.0, dtype=torch.float64, device=DEV) for _ in range(3)]  # the allocator hands the block back
    torch.cuda.current_stream().synchronize()
    assert torch.equal(bits(p.to_torch()), bits(want))
    del junk
    # export, drop the handle, let the library reuse its blocks: the exported tensor keeps its values
    q = TP.from_torch(want) * TP.from_scalar(2.0)
    ref = q.array()
    out = q.to_torch()
    del q
    for k in range(4):
        r = TP.from_torch(rand_bits(full, 40 + k)) + TP.from_torch(rand_bits(full, 50 + k))
        r.array()
    assert np.array_equal(out.cpu().numpy().view(np.int64), ref.view(np.int64))


def test_no_host_transfer_on_the_device_path():
    import genfer_amd

    TP = genfer_amd.TaylorPoly
    x = torch.rand((128, 128, 128), dtype=torch.float64, device=DEV)
    y = torch.rand((2, 2, 2), dtype=torch.float64, device=DEV)
    m0 = genfer_amd.op_stats()["host_to_device_mirrors"]
    z = (TP.from_torch(x) * TP.from_torch(y, (128, 128, 128))).to_torch()
    torch.cuda.synchronize()
    assert genfer_amd.op_stats()["host_to_device_mirrors"] == m0
    assert z.shape == (128, 128, 128)


# ---- refusals -------------------------------------------------------------------------------------------------------------


def test_refusals_name_the_problem():
    import genfer_amd
    from genfer_amd.taylor import TaylorError

    TP, TPI = genfer_amd.TaylorPoly, genfer_amd.IntervalTaylorPoly
    with pytest.raises(TaylorError, match="on cpu"):
        TP.from_torch(torch.zeros((3, 4), dtype=torch.float64))
    with pytest.raises(TaylorError, match="float32"):
        TP.from_torch(torch.zeros((3, 4), dtype=torch.float32, device=DEV))
    # pinned host memory through the C entry point itself
    pinned = torch.zeros(16, dtype=torch.float64).pin_memory()
    sh, dg = (ctypes.c_size_t * 1)(16), (ctypes.c_size_t * 1)(16)
    fn = TP._fn
    assert not fn.from_device(ctypes.c_void_p(pinned.data_ptr()), None, sh, dg, 1, None)
    assert "pinned host memory" in fn.last_error().decode()
    assert not fn.from_device(None, None, sh, dg, 1, None)
    assert "null pointer" in fn.last_error().decode()
    # shape / degrees: the text of from_host
    with pytest.raises(TaylorError) as host_err:
        TP.new(np.zeros((4, 5)), (3, 5))
    with pytest.raises(TaylorError) as dev_err:
        TP.from_torch(torch.zeros((4, 5), dtype=torch.float64, device=DEV), (3, 5))
    assert str(dev_err.value) == str(host_err.value) and "invariant violated" in str(dev_err.value)
    p = TP.from_torch(torch.rand((4, 5), dtype=torch.float64, device=DEV))
    with pytest.raises(TaylorError, match="overlap"):
        p.to_torch(out=torch.empty(8, dtype=torch.float64, device=DEV).as_strided((4, 5), (1, 1)))
    with pytest.raises(TaylorError, match="zero stride"):
        p.to_torch(out=torch.empty((1, 5), dtype=torch.float64, device=DEV).expand(4, 5))
    with pytest.raises(TaylorError, match="shape"):
        p.to_torch(out=torch.empty((5, 4), dtype=torch.float64, device=DEV))
    with pytest.raises(TaylorError, match=r"stacked as \[2"):
        TPI.from_torch(torch.zeros((3, 4), dtype=torch.float64, device=DEV))
