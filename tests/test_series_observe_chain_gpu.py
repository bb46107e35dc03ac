"""The fused observation chain on the MI355X: observe_chain of genfer_amd.series, series2, interval_series, interval_series2
(gft[i]_series_observe_chain / gft[i]_series2_observe_chain).

Every coefficient of every item carries the oracle's bits (OTP / OTPI observe_chain per item; derive_scale step by step for the
continuous form) on data without exact zeros: both sides of the form switch at 64 coefficients, every layout of a, x and cs, out=,
the forms against each other, the limits.  Where the reference's Mul looks at the data (exact zeros, a zero constant) and for
non-finite values the yardstick is the numpy model of tests/_series_observe_chain_model.py, itself held to the oracle by the CPU
tests."""
import ctypes as C

import numpy as np
import pytest

import _series_observe_chain_model as CM
import _series_observe_model as M
from _series2_oracle import assert_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
LENGTHS = [(4,), (9,), (33,), (64,), (65,), (130,)]
SHAPES = [(5, 7), (7, 5), (1, 9), (9, 1), (3, 66), (66, 3), (12, 12)]
BATCH = (3, 2)
XS = np.array([[0.0, -0.0], [1.0, 0.3], [-1.7, 2.5]])  # per item: both zeros, one, ordinary values


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd
    from genfer_amd import series

    genfer_amd.init(0)
    yield
    series.set_form(None)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def module(rank, interval):
    from genfer_amd import interval_series, interval_series2, series, series2

    return {(1, False): series, (2, False): series2, (1, True): interval_series, (2, True): interval_series2}[(rank, interval)]


def values(shape, seed, interval):
    """uniform in [-0.5, 0.5) without exact zeros; intervals [v, v + w] with 0 < w < 1e-3 that do not reach zero"""
    rng = np.random.default_rng(seed)
    v = rng.random(shape) - 0.5
    v[v == 0.0] = 0.25
    if not interval:
        return v
    hi = v + rng.random(shape) * 1e-3 * np.abs(v) + 1e-12 * np.abs(v)
    return np.stack([v, hi])


def scalars(xs, interval):
    """the scalars x: points at 0, -0 and 1, a width on the others"""
    xs = np.asarray(xs, dtype=np.float64)
    if not interval:
        return xs
    plain = (xs != 0.0) & (xs != 1.0)
    return np.stack([xs, np.where(plain, xs + 1e-3, xs)])


def constants(shape, seed, interval):
    """cs in [0.25, 1.25) with a 1.0 at step 0 of every other item and in the middle of the chain of the first"""
    rng = np.random.default_rng(seed)
    c = 0.25 + rng.random(shape)
    flat = c.reshape(-1, shape[-1])
    flat[1::2, 0] = 1.0
    flat[0, shape[-1] // 2] = 1.0
    if not interval:
        return c
    hi = c * (1.0 + 1e-6)
    hi[c == 1.0] = 1.0
    return np.stack([c, hi])


def chains(length):
    """(nsteps, degree_p1): nsteps in {1, 2, 5, L - 2}, degree_p1 in {2, 3, L - nsteps}, where the shape rules admit them"""
    return [(n, d) for n in sorted({1, 2, 5, length - 2}) for d in sorted({2, 3, length - n}) if n >= 1 and d >= 2 and d + n <= length]


def call(mod, a, var, x, cs, d, rank, **kw):
    return mod.observe_chain(a, *(() if rank == 1 else (var,)), x, cs, d, **kw)


def layouts(seed, item, n, interval):
    """(a, x, cs) four ways over the batch [3, 2]: contiguous; stride 0 (a over batch axis 0, x over axis 1, cs over axis 0, left to
    the call's own broadcast); sliced from wider tensors (a row stride, a stride on x, wider rows of cs); transposed batch axes"""
    lead = (2,) if interval else ()
    p = len(lead)
    wide = item[:-1] + (item[-1] + 3,)
    t = lambda v: dev(v).transpose(p, p + 1)  # noqa: E731
    out = {
        "contiguous": (dev(values(BATCH + item, seed, interval)), dev(scalars(XS, interval)), dev(constants(BATCH + (n,), seed + 1, interval))),
        "stride 0": (dev(values((1, BATCH[1]) + item, seed + 2, interval)).expand(lead + BATCH + item), dev(scalars(XS[:, :1], interval)),
                     dev(constants((BATCH[1], n), seed + 3, interval))),
        "sliced": (dev(values(BATCH + wide, seed + 4, interval))[..., 1:1 + item[-1]], dev(scalars(np.repeat(XS, 2, axis=1), interval))[..., ::2],
                   dev(constants(BATCH + (n + 3,), seed + 5, interval))[..., 1:1 + n]),
        "transposed": (t(values((BATCH[1], BATCH[0]) + item, seed + 6, interval)), t(scalars(XS.T, interval)),
                       dev(constants((BATCH[1], BATCH[0], n), seed + 7, interval)).transpose(p, p + 1)),
    }
    a, x, cs = out["stride 0"]
    assert a.stride(p) == 0 and x.shape[-1] == 1 and cs.dim() == p + 2
    assert out["sliced"][1].stride(-1) == 2 and out["sliced"][2].stride(-2) == n + 3 and not out["transposed"][0].is_contiguous()
    return out


def expected(T, a, item, var, x, cs, d, interval):
    """the oracle per item on the host copies (x None: the continuous form)"""
    an, cn = a.cpu().numpy(), cs.cpu().numpy()
    return CM.oracle_chain(T, an, item, var, None if x is None else x.cpu().numpy(), cn, d, interval)


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("item", LENGTHS + SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_exact_against_the_oracle(item, interval, OTP, OTPI):
    from genfer_amd import series

    rank = len(item)
    mod, T = module(rank, interval), OTPI if interval else OTP
    checked = 0
    for var in ((0,) if rank == 1 else (0, 1)):
        L = item[var]
        for n, d in chains(L):
            for name, (a, x, cs) in layouts(1000 * item[0] + 10 * item[-1] + n, item, n, interval).items():
                got = call(mod, a, var, x, cs, d, rank)
                assert series.last_form() == ("A" if L <= 64 else "B")
                assert_bits(got, expected(T, a, item, var, x, cs, d, interval), f"{item} var={var} nsteps={n} degree_p1={d} {name}")
                checked += 1
                if name in ("contiguous", "sliced"):  # the continuous form: derive_scale step by step
                    got = call(mod, a, var, None, cs, d, rank)
                    assert_bits(got, expected(T, a, item, var, None, cs, d, interval), f"{item} var={var} nsteps={n} degree_p1={d} {name} continuous")
            # degree_p1 defaults to L - nsteps
            a, x, cs = layouts(7, item, n, interval)["contiguous"]
            assert call(mod, a, var, x, cs, None, rank).shape[-rank:] == CM.result_shape(item, var, L - n)
    assert checked >= 4 or min(item) == 1


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_out_views_and_overlaps(interval, OTP, OTPI):
    """out= into a strided view with the guard around it untouched; a result inside a, x or cs is refused"""
    from genfer_amd.taylor import TaylorError

    T, lead = (OTPI if interval else OTP), ((2,) if interval else ())
    for item, var, n, d in (((9,), 0, 2, 5), ((5, 7), 1, 3, 4), ((7, 5), 0, 2, 3), ((66, 3), 0, 5, 61)):
        rank = len(item)
        mod = module(rank, interval)
        a, x, cs = layouts(50 + rank, item, n, interval)["contiguous"]
        res = CM.result_shape(item, var, d)
        buf = torch.full(lead + (BATCH[0], 2 * BATCH[1]) + res[:-1] + (res[-1] + 2,), -7.0, dtype=torch.float64, device=DEV)
        view = buf[..., ::2, :, 1:1 + res[-1]] if rank == 2 else buf[..., ::2, 1:1 + res[-1]]
        assert call(mod, a, var, x, cs, d, rank, out=view) is view
        assert_bits(view, expected(T, a, item, var, x, cs, d, interval), f"{item} out=view")
        mask = torch.ones_like(buf, dtype=torch.bool)
        (mask[..., ::2, :, 1:1 + res[-1]] if rank == 2 else mask[..., ::2, 1:1 + res[-1]]).fill_(False)
        assert (buf[mask] == -7.0).all()
        n_out = int(np.prod(lead + BATCH + res))
        for who, t in (("a", a), ("x", x), ("cs", cs)):
            flat = torch.zeros(t.numel() + n_out + 8, dtype=torch.float64, device=DEV)
            inside = flat[:t.numel()].view(t.shape).copy_(t)
            args = {"a": a, "x": x, "cs": cs, who: inside}
            with pytest.raises(TaylorError, match=f"partially overlaps {who}"):
                call(mod, args["a"], var, args["x"], args["cs"], d, rank, out=flat[1:1 + n_out].view(lead + BATCH + res))


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_the_two_forms_give_the_same_bits(interval):
    """series_form 1 and 2 on lines of at most 64 coefficients: identical bits; gft_series_last_form() reports the form; beyond 64
    form A falls back to form B"""
    from genfer_amd import series

    try:
        for item, var, n, d in (((9,), 0, 5, 3), ((64,), 0, 62, 2), ((33,), 0, 2, 31), ((5, 7), 1, 2, 5), ((12, 12), 0, 5, 7), ((3, 66), 0, 1, 2)):
            rank = len(item)
            mod = module(rank, interval)
            a, x, cs = layouts(80 + rank, item, n, interval)["sliced"]
            got = {}
            for form in ("A", "B"):
                series.set_form(form)
                got[form] = (call(mod, a, var, x, cs, d, rank), call(mod, a, var, None, cs, d, rank))
                assert series.last_form() == form
            for u, v in zip(got["A"], got["B"]):
                assert torch.equal(u.view(torch.int64), v.view(torch.int64)), (item, var, n, d)
        series.set_form("A")
        a, x, cs = layouts(90, (65,), 3, interval)["contiguous"]
        call(module(1, interval), a, 0, x, cs, 2, 1)
        assert series.last_form() == "B"
    finally:
        series.set_form(None)


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_against_the_model_where_the_oracle_is_no_yardstick(interval):
    """data with +-0, inf and NaN, a zero constant in the middle of a chain (the item is all +0.0), -0.0 as a constant, non-finite
    scalars: the stated loops, bit for bit, in both forms' ranges"""
    A = M.IV if interval else M.F64
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0])
    for item, var, n, d in (((12,), 0, 4, 3), ((70,), 0, 5, 9), ((6, 9), 1, 3, 4), ((9, 6), 0, 3, 4), ((2, 70), 1, 4, 60)):
        rank = len(item)
        mod = module(rank, interval)
        rng = np.random.default_rng(5 + item[0])
        a = rng.random((8,) + item) - 0.5
        pick = rng.random(a.shape) < 0.3
        a[pick] = rng.choice(special, size=int(pick.sum()))
        x = np.array([0.3, 0.0, -0.0, 1.0, np.inf, np.nan, -2.0, 0.5])
        cs = 0.25 + rng.random((8, n))
        cs[0, n // 2] = 0.0       # the item is all +0.0
        cs[1, n - 1] = -0.0       # -0.0 counts as zero, in the last step too
        cs[2, 0] = np.inf
        cs[3, 1] = np.nan
        cs[4, 0] = 1.0
        cs[5, n // 2] = -1.0
        if interval:
            a, x, cs = np.stack([a, a]), np.stack([x, x]), np.stack([cs, cs])
            a[1, 6], x[1, 6], cs[1, 6] = a[0, 6] + 0.25, x[0, 6] + 0.5, cs[0, 6] * 1.5  # one item of wide intervals
        axis = -1 if rank == 1 else var - 2
        for xx in (x, None):
            got = call(mod, dev(a), var, None if xx is None else dev(xx), dev(cs), d, rank)
            want = CM.observe_chain(A, a, axis, xx, cs, d, rank)
            assert_bits(got, want, f"{item} var={var} x={'given' if xx is not None else None}")
            g = got.cpu().numpy()
            zero = g[:, :2] if interval else g[:2]
            assert (zero == 0.0).all() and not np.signbit(zero).any()


def test_point_intervals_through_plane_stride_0(OTPI):
    """a.expand(2, ...), x.expand(2, ...) and cs.expand(2, ...) are point intervals: plane stride 0, no copy"""
    for item, var, n, d in (((9,), 0, 2, 7), ((5, 7), 1, 3, 3), ((66, 3), 0, 4, 62)):
        rank = len(item)
        mod = module(rank, True)
        a, x, cs = (t.expand((2,) + tuple(t.shape)) for t in layouts(60 + rank, item, n, False)["contiguous"])
        assert a.stride(0) == 0 and x.stride(0) == 0 and cs.stride(0) == 0
        assert_bits(call(mod, a, var, x, cs, d, rank), expected(OTPI, a, item, var, x, cs, d, True), f"{item} var={var}")


def test_the_limits(OTP, OTPI):
    """(3, 4096) with 64 steps and (2, 64, 64) with 16 steps run and carry the oracle's bits, the interval limits likewise; one
    coefficient more is refused"""
    from genfer_amd import interval_series, interval_series2, series, series2
    from genfer_amd.taylor import TaylorError

    a, x, cs = dev(values((3, 4096), 5, False)), dev(np.array([0.3, 0.0, 1.0])), dev(constants((3, 64), 6, False))
    assert_bits(series.observe_chain(a, x, cs), expected(OTP, a, (4096,), 0, x, cs, 4032, False), "4096, 64 steps")
    a, x, cs = dev(values((2, 64, 64), 7, False)), dev(np.array([0.3, -1.7])), dev(constants((2, 16), 8, False))
    for var in (0, 1):
        assert_bits(series2.observe_chain(a, var, x, cs), expected(OTP, a, (64, 64), var, x, cs, 48, False), f"64x64 var={var}, 16 steps")
    a, x, cs = dev(values((2, 2048), 9, True)), dev(scalars([0.3, 1.0], True)), dev(constants((2, 64), 10, True))
    assert_bits(interval_series.observe_chain(a, x, cs), expected(OTPI, a, (2048,), 0, x, cs, 1984, True), "interval 2048, 64 steps")
    a, x, cs = dev(values((2, 32, 64), 11, True)), dev(scalars([0.3, -1.7], True)), dev(constants((2, 16), 12, True))
    assert_bits(interval_series2.observe_chain(a, 1, x, cs), expected(OTPI, a, (32, 64), 1, x, cs, 48, True), "interval 32x64, 16 steps")
    ones = lambda *s: torch.ones(s, dtype=torch.float64, device=DEV)  # noqa: E731
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series.observe_chain(ones(1, 4097), ones(1), ones(1, 2))
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series2.observe_chain(ones(1, 64, 65), 1, ones(1), ones(1, 2))
    with pytest.raises(TaylorError, match="exceeds the limit of 2048"):
        interval_series.observe_chain(ones(2, 1, 2049), ones(2, 1), ones(2, 1, 2))


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_seventy_thousand_items(interval):
    """more lines than the launches have places for, so both kernels stride over them: 70 000 items of length 6 (form B caps at
    65 536 workgroups) and of (4, 6) with four lines each (form A caps at 262 144 waves), against the vectorised model"""
    from genfer_amd import series

    A = M.IV if interval else M.F64
    B = 70000
    try:
        for item, var, n, d in (((6,), 0, 3, 3), ((4, 6), 1, 2, 4)):
            rank = len(item)
            mod = module(rank, interval)
            a = values((B,) + item, 70 + rank, interval)
            x = scalars(np.resize(XS.reshape(-1), B), interval)
            cs = constants((B, n), 71, interval)
            want = CM.observe_chain(A, a, -1, x, cs, d, rank)
            for form in ("A", "B"):
                series.set_form(form)
                assert_bits(call(mod, dev(a), var, dev(x), dev(cs), d, rank), want, f"{item} form {form}")
    finally:
        series.set_form(None)


def test_the_library_refuses_by_itself():
    """the C entry points judge nsteps, degree_p1 and the result's shape themselves, by name, and write nothing"""
    from genfer_amd import series

    L = series._lib()
    a = torch.ones((2, 9), dtype=torch.float64, device=DEV)
    x, cs = torch.ones(2, dtype=torch.float64, device=DEV), torch.ones((2, 3), dtype=torch.float64, device=DEV)
    out = torch.full((2, 9), -7.0, dtype=torch.float64, device=DEV)
    bsz, rbs = (C.c_size_t * 1)(2), (C.c_int64 * 1)(9)  # the result's items lie 9 apart
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = lambda n, d, m: (p(a), None, 9, p(x), None, p(cs), None, n, d, p(out), rbs, m, bsz, 1, None)  # noqa: E731
    for (n, d, m), text in (((3, 1, 1), "degree_p1 = 1"), ((0, 3, 3), "nsteps = 0"), ((3, 7, 7), "degree_p1 + nsteps = 7 + 3, but a has 9"),
                            ((3, 6, 5), "the result has 5 coefficients; with degree_p1 = 6 it has 6")):
        assert L.gft_series_observe_chain(*args(n, d, m)) != 0
        assert text in L.gft_last_error().decode(), L.gft_last_error().decode()
    assert L.gft_series2_observe_chain(p(a), None, 9, 1, 9, 2, p(x), None, p(cs), None, 3, 6, p(out), None, 6, 1, 6, bsz, 1, None) != 0
    assert "var = 2" in L.gft_last_error().decode()
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert L.gft_series_observe_chain(*args(3, 6, 6)) == 0  # and the same call within the rules runs
    torch.cuda.synchronize()
    assert (out[:, :6] != -7.0).all() and (out[:, 6:] == -7.0).all()
