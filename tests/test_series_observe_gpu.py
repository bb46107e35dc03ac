"""The batched observation ops on the MI355X: derivative, taylor_expansion_of_coeff, shift_down, evaluate_all_one of genfer_amd.series,
series2, interval_series, interval_series2 (gft_series_* / gft_series2_* and their gfti_ twins) and the differentiable twins in
series and series2_grad.

Every coefficient of every item carries the oracle's bits (OTP / OTPI per item; evaluate_all_one, which the handle API does not
have, against the ordered fold of tests/_series_observe_model.py, itself held to the plain-Python fold by the CPU tests): views,
stride-0 broadcasts, row strides, transposed batches, out=, the same view at k = 0, refused overlaps, special values, the limits,
a batch beyond 65 535 items, and the gradients."""
import numpy as np
import pytest

import _series_observe_model as M
from _series2_oracle import assert_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
OPS3 = ("derivative", "taylor_expansion_of_coeff", "shift_down")
LENGTHS = [(1,), (2,), (7,), (8,), (9,), (17,)]
SHAPES = [(1, 6), (6, 1), (9, 1), (17, 1), (3, 5), (8, 8), (4, 17), (12, 7), (2, 33)]
BATCH = (3, 2)


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield


def dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_() if grad else t


def module(rank, interval):
    from genfer_amd import interval_series, interval_series2, series, series2

    return {(1, False): series, (2, False): series2, (1, True): interval_series, (2, True): interval_series2}[(rank, interval)]


def orders(length):
    return sorted({k for k in (0, 1, 7, 8, 9, length - 1) if 0 <= k < length})


def values(kind, shape, seed, interval):
    """dense: 0.5 + uniform; mixed: uniform - 0.5; intervals [v, v + w] with 0 < w < 1e-3"""
    rng = np.random.default_rng(seed)
    v = 0.5 + rng.random(shape) if kind == "dense" else rng.random(shape) - 0.5
    return np.stack([v, v + rng.random(shape) * 1e-3 + 1e-9]) if interval else v


def call(mod, op, x, var, k, rank, **kw):
    if op == "evaluate_all_one":
        return mod.evaluate_all_one(x, **kw)
    return getattr(mod, op)(x, *(() if rank == 1 else (var,)), k, **kw)


def expected(T, op, xn, item, var, k, interval):
    """the oracle per item (evaluate_all_one: the model's fold); xn is the numpy operand [(2,) B..., item]"""
    rank = len(item)
    if op == "evaluate_all_one":
        return M.evaluate_all_one(M.IV if interval else M.F64, xn, rank)
    lead = 1 if interval else 0
    batch = xn.shape[lead:xn.ndim - rank]
    flat = xn.reshape(xn.shape[:lead] + (-1,) + item)
    outs = [getattr(T.new(flat[:, b] if interval else flat[b], item), op)(var, k).array() for b in range(flat.shape[lead])]
    w = np.stack(outs, axis=lead)
    return w.reshape(w.shape[:lead] + batch + w.shape[lead + 1:])


def layouts(kind_seed, item, interval):
    """the operand four ways, all of batch [3, 2]: contiguous, broadcast through stride 0 (batch [1, 2] expanded), sliced from a
    wider tensor (row stride > n1, and a batch stride to match), and with transposed batch axes"""
    lead = (2,) if interval else ()
    wide = item[:-1] + (item[-1] + 3,)
    a = dev(values("dense", BATCH + item, kind_seed, interval))
    b = dev(values("mixed", (1, BATCH[1]) + item, kind_seed + 1, interval)).expand(lead + BATCH + item)
    c = dev(values("mixed", BATCH + wide, kind_seed + 2, interval))[..., 1:1 + item[-1]]
    d = dev(values("dense", (BATCH[1], BATCH[0]) + item, kind_seed + 3, interval)).transpose(len(lead), len(lead) + 1)
    assert b.stride(len(lead)) == 0 and c.stride(-2) == item[-1] + 3 and not d.is_contiguous()
    return {"contiguous": a, "stride 0": b, "sliced": c, "transposed": d}


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("item", LENGTHS + SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_exact_against_the_oracle(item, interval, OTP, OTPI):
    rank = len(item)
    mod, T = module(rank, interval), OTPI if interval else OTP
    checked = 0
    for name, x in layouts(1000 * item[0] + item[-1], item, interval).items():
        xn = x.cpu().numpy()
        assert_bits(mod.evaluate_all_one(x), expected(T, "evaluate_all_one", xn, item, None, None, interval), f"evaluate_all_one {item} {name}")
        for op in OPS3:
            for var in ((0,) if rank == 1 else (0, 1)):
                for k in orders(item[var]):
                    got = call(mod, op, x, var, k, rank)
                    assert_bits(got, expected(T, op, xn, item, var, k, interval), f"{op} {item} var={var} k={k} {name}")
                    checked += 1
    assert checked >= 4 * 3


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_out_views_and_aliasing(interval, OTP, OTPI):
    """out= into a strided view (the guard around it untouched), the operand itself as the same view at k = 0, a partial overlap
    refused"""
    from genfer_amd.taylor import TaylorError

    T, lead = (OTPI if interval else OTP), ((2,) if interval else ())
    for item, var, k in (((9,), 0, 4), ((4, 17), 1, 9), ((12, 7), 0, 5)):
        rank = len(item)
        mod = module(rank, interval)
        x = dev(values("mixed", BATCH + item, 7 + rank, interval))
        xn = x.cpu().numpy()
        for op in OPS3:
            res = list(item)
            res[var] -= k
            buf = torch.full(lead + (BATCH[0], 2 * BATCH[1]) + tuple(res[:-1]) + (res[-1] + 2,), -7.0, dtype=torch.float64, device=DEV)
            view = buf[..., ::2, :, 1:1 + res[-1]] if rank == 2 else buf[..., ::2, 1:1 + res[-1]]
            assert call(mod, op, x, var, k, rank, out=view) is view
            assert_bits(view, expected(T, op, xn, item, var, k, interval), f"{op} {item} out=view")
            mask = torch.ones_like(buf, dtype=torch.bool)
            (mask[..., ::2, :, 1:1 + res[-1]] if rank == 2 else mask[..., ::2, 1:1 + res[-1]]).fill_(False)
            assert (buf[mask] == -7.0).all()
            # the same view at k = 0
            y = x.clone()
            assert call(mod, op, y, var, 0, rank, out=y) is y
            assert_bits(y, expected(T, op, xn, item, var, 0, interval), f"{op} {item} in place")
            # a partial overlap: the result one element into the operand's memory
            if k > 0:
                n_out = int(np.prod(lead + BATCH + tuple(res)))
                flat = torch.zeros(x.numel() + 8, dtype=torch.float64, device=DEV)
                xo = flat[:x.numel()].view(x.shape).copy_(x)
                with pytest.raises(TaylorError, match="partially overlaps"):
                    call(mod, op, xo, var, k, rank, out=flat[1:1 + n_out].view(lead + BATCH + tuple(res)))
        ev = torch.full(lead + (BATCH[0], 2 * BATCH[1]), -7.0, dtype=torch.float64, device=DEV)
        mod.evaluate_all_one(x, out=ev[..., ::2])
        assert_bits(ev[..., ::2], expected(T, "evaluate_all_one", xn, item, None, None, interval), "evaluate_all_one out=view")
        assert (ev[..., 1::2] == -7.0).all()


def test_special_values(OTP):
    """one item with inf, NaN and -0.0 beside an ordinary one: the oracle's bits (a NaN where it has a NaN), the neighbour untouched"""
    from genfer_amd import series, series2

    row = np.array([-0.0, 1.5, np.inf, -2.0, np.nan, -0.0, 3.0, -np.inf, 0.25, -0.0, 1.0, 2.0])
    x1 = np.stack([row, np.linspace(0.5, 1.5, 12)])
    for k in (0, 1, 5, 8, 11):
        for op in OPS3:
            assert_bits(getattr(series, op)(dev(x1), k), expected(OTP, op, x1, (12,), 0, k, False), f"{op} k={k}")
    assert_bits(series.evaluate_all_one(dev(x1)), M.evaluate_all_one(M.F64, x1, 1), "evaluate_all_one")
    x2 = x1.reshape(2, 3, 4)
    for var in (0, 1):
        for k in range((3, 4)[var]):
            for op in OPS3:
                assert_bits(getattr(series2, op)(dev(x2), var, k), expected(OTP, op, x2, (3, 4), var, k, False), f"{op} var={var} k={k}")
    got = series.shift_down(dev(np.array([[-0.0, -0.0]])), 0).cpu().numpy()
    assert not np.signbit(got[0, 0]) and np.signbit(got[0, 1])  # x[0] + 0.0 is +0.0; the copy keeps its sign


def test_the_limits(OTP):
    """nx = 4096 with B = 3 and (64, 64) with B = 2 run and carry the oracle's bits; one coefficient more is refused"""
    from genfer_amd import series, series2
    from genfer_amd.taylor import TaylorError

    x = values("dense", (3, 4096), 5, False)
    tx = dev(x)
    for op in OPS3:
        for k in (2048, 4095):
            assert_bits(getattr(series, op)(tx, k), expected(OTP, op, x, (4096,), 0, k, False), f"{op} 4096 k={k}")
    assert_bits(series.evaluate_all_one(tx), M.evaluate_all_one(M.F64, x, 1), "evaluate_all_one 4096")
    y = values("mixed", (2, 64, 64), 6, False)
    ty = dev(y)
    for op in OPS3:
        for var in (0, 1):
            for k in (32, 63):
                assert_bits(getattr(series2, op)(ty, var, k), expected(OTP, op, y, (64, 64), var, k, False), f"{op} 64x64 var={var} k={k}")
    assert_bits(series2.evaluate_all_one(ty), M.evaluate_all_one(M.F64, y, 2), "evaluate_all_one 64x64")
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series.derivative(torch.ones((1, 4097), dtype=torch.float64, device=DEV), 1)
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series2.shift_down(torch.ones((1, 64, 65), dtype=torch.float64, device=DEV), 0, 1)


def test_the_library_refuses_by_itself():
    """the C entry points judge k, var and the result's shape themselves, naming k and the length, before anything is launched"""
    import ctypes as C

    from genfer_amd import series

    L = series._lib()
    x = torch.ones((2, 6), dtype=torch.float64, device=DEV)
    out = torch.full((2, 6), -7.0, dtype=torch.float64, device=DEV)
    bsz = (C.c_size_t * 1)(2)
    args = lambda k, n: (C.c_void_p(x.data_ptr()), None, 6, k, C.c_void_p(out.data_ptr()), None, n, bsz, 1, None)  # noqa: E731
    assert L.gft_series_derivative(*args(6, 1)) != 0
    msg = L.gft_last_error().decode()
    assert "k = 6" in msg and "6 stored coefficients" in msg
    assert L.gft_series_shift_down(*args(2, 5)) != 0 and "the result has 5 coefficients" in L.gft_last_error().decode()
    torch.cuda.synchronize()
    assert (out == -7.0).all()


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_seventy_thousand_items(interval):
    """more items than a grid dimension of 65 535 holds, n = 4 and (2, 2), against the vectorised model"""
    A = M.IV if interval else M.F64
    for item in ((4,), (2, 2)):
        rank = len(item)
        mod = module(rank, interval)
        x = values("mixed", (70000,) + item, 70 + rank, interval)
        tx = dev(x)
        assert_bits(mod.evaluate_all_one(tx), M.evaluate_all_one(A, x, rank), f"evaluate_all_one {item}")
        for var in ((0,) if rank == 1 else (0, 1)):
            ax = -1 if rank == 1 else var - 2
            for k in range(item[var]):
                assert_bits(call(mod, "derivative", tx, var, k, rank), M.derivative(A, x, ax, k), f"derivative {item} var={var} k={k}")
                assert_bits(call(mod, "taylor_expansion_of_coeff", tx, var, k, rank), M.taylor_expansion_of_coeff(A, x, ax, k), f"coeff {item} var={var} k={k}")
                assert_bits(call(mod, "shift_down", tx, var, k, rank), M.shift_down(A, x, ax, k, rank), f"shift_down {item} var={var} k={k}")


def test_point_intervals_through_plane_stride_0(OTPI):
    """x.expand(2, ...) is a batch of point intervals: plane stride 0, no copy"""
    for item in ((9,), (4, 17)):
        rank = len(item)
        mod = module(rank, True)
        p = dev(values("mixed", BATCH + item, 90 + rank, False))
        x = p.expand((2,) + tuple(p.shape))
        assert x.stride(0) == 0
        xn = x.cpu().numpy()
        assert_bits(mod.evaluate_all_one(x), expected(OTPI, "evaluate_all_one", xn, item, None, None, True), "evaluate_all_one")
        for op in OPS3:
            for var in ((0,) if rank == 1 else (0, 1)):
                for k in (0, item[var] // 2, item[var] - 1):
                    assert_bits(call(mod, op, x, var, k, rank), expected(OTPI, op, xn, item, var, k, True), f"{op} {item} var={var} k={k}")


# ---- autograd ----------------------------------------------------------------------------------------------------------------------


def grad_module(rank):
    from genfer_amd import series, series2_grad

    return series if rank == 1 else series2_grad


def ints(shape, seed):
    return np.random.default_rng(seed).integers(-3, 4, size=shape).astype(np.float64)


@pytest.mark.parametrize("item", [(6,), (5, 4)], ids=str)
def test_propagation_and_forward_bits(item):
    """a grad_fn exactly when grad mode is on and the operand requires grad; the forward bits are the raw call's"""
    rank = len(item)
    mod, raw = grad_module(rank), module(rank, False)
    xa = values("mixed", BATCH + item, 21, False)
    for op in OPS3 + ("evaluate_all_one",):
        for var in ((0,) if rank == 1 else (0, 1)):
            k = item[var] // 2
            plain = call(raw, op, dev(xa), var, k, rank)
            x = dev(xa, True)
            z = call(mod, op, x, var, k, rank)
            assert z.requires_grad and z.grad_fn is not None
            assert torch.equal(z.detach().view(torch.int64), plain.view(torch.int64))
            assert not call(mod, op, dev(xa), var, k, rank).requires_grad
            with torch.no_grad():
                assert not call(mod, op, x, var, k, rank).requires_grad


@pytest.mark.parametrize("item", [(6,), (7,), (5, 4), (7, 1), (1, 7)], ids=str)
def test_gradients_exact_on_integers(item):
    """gx[k + j] = g[j] * factor_j and +0.0 below k; shift_down: gx[i] = g[0] for i <= k, gx[k + j] = g[j]; evaluate_all_one: g over the
    item -- against the formulas in numpy (tests/_series_observe_model.py), torch.equal"""
    rank = len(item)
    mod = grad_module(rank)
    xa = ints(BATCH + item, 31)
    for var in ((0,) if rank == 1 else (0, 1)):
        ax = -1 if rank == 1 else var - 2
        for k in range(item[var]):
            for op, name in (("derivative", "derivative"), ("taylor_expansion_of_coeff", "coeff"), ("shift_down", None)):
                x = dev(xa, True)
                z = call(mod, op, x, var, k, rank)
                ga = ints(tuple(z.shape), 37 + k)
                z.backward(dev(ga))
                want = M.shift_down_adj(ga, ax, k) if name is None else M.scaled_adj(name, ga, ax, k)
                assert torch.equal(x.grad, dev(want)), (op, item, var, k)
                if name is not None and k:
                    assert not torch.signbit(x.grad.movedim(ax, -1)[..., :k]).any()
    x = dev(xa, True)
    z = mod.evaluate_all_one(x)
    ga = ints(tuple(z.shape), 41)
    z.backward(dev(ga))
    assert torch.equal(x.grad, dev(M.evaluate_all_one_adj(ga, item)))


def test_gradients_of_broadcast_operands_are_reduced():
    """an operand broadcast over a batch axis (stride 0) receives the sum over that axis"""
    from genfer_amd import series

    w = dev(ints((5,), 43), True)
    x = w.expand(3, 5)
    z = series.derivative(x, 1)
    ga = ints((3, 4), 44)
    z.backward(dev(ga))
    assert torch.equal(w.grad, dev(M.scaled_adj("derivative", ga, -1, 1).sum(0)))


@pytest.mark.parametrize("item", [(5,), (3, 4)], ids=str)
def test_gradcheck(item):
    rank = len(item)
    mod = grad_module(rank)
    xa = values("dense", (2,) + item, 51, False)
    for var in ((0,) if rank == 1 else (0, 1)):
        for k in (0, 1, item[var] - 1):
            for op in OPS3:
                assert torch.autograd.gradcheck(lambda a: call(mod, op, a, var, k, rank), (dev(xa, True),)), (op, var, k)
    assert torch.autograd.gradcheck(lambda a: mod.evaluate_all_one(a), (dev(xa, True),))


def test_tracked_operands_are_refused_where_they_must_be():
    from genfer_amd import interval_series, interval_series2, series, series2, series2_grad
    from genfer_amd.taylor import TaylorError

    x1, x2 = dev(values("dense", (3, 6), 61, False), True), dev(values("dense", (3, 4, 6), 62, False), True)
    for op in OPS3:
        with pytest.raises(TaylorError, match="out= cannot be combined with an operand that requires grad"):
            getattr(series, op)(x1, 2, out=torch.empty((3, 4), dtype=torch.float64, device=DEV))
        with pytest.raises(TaylorError, match="out= cannot be combined with an operand that requires grad"):
            getattr(series2_grad, op)(x2, 1, 2, out=torch.empty((3, 4, 4), dtype=torch.float64, device=DEV))
        with pytest.raises(TaylorError, match="this version of series2 has no autograd"):
            getattr(series2, op)(x2, 1, 2)
    with pytest.raises(TaylorError, match="out= cannot be combined"):
        series.evaluate_all_one(x1, out=torch.empty(3, dtype=torch.float64, device=DEV))
    with pytest.raises(TaylorError, match="this version of series2 has no autograd"):
        series2.evaluate_all_one(x2)
    i1 = torch.stack([x1.detach(), x1.detach() + 1e-3]).requires_grad_()
    i2 = torch.stack([x2.detach(), x2.detach() + 1e-3]).requires_grad_()
    for op in OPS3:
        with pytest.raises(TaylorError, match="this version of interval_series has no autograd"):
            getattr(interval_series, op)(i1, 2)
        with pytest.raises(TaylorError, match="this version of interval_series2 has no autograd"):
            getattr(interval_series2, op)(i2, 0, 2)
    with pytest.raises(TaylorError, match="this version of interval_series has no autograd"):
        interval_series.evaluate_all_one(i1)
    with pytest.raises(TaylorError, match="this version of interval_series2 has no autograd"):
        interval_series2.evaluate_all_one(i2)
    with torch.no_grad():  # grad mode off: plain calls
        assert not series2.derivative(x2, 1, 2).requires_grad and not interval_series.shift_down(i1, 2).requires_grad
