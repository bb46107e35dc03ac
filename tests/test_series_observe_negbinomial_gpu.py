"""The fused negative-binomial observation and the Lah row on the MI355X: observe_negbinomial of genfer_amd.series, series2,
interval_series, interval_series2 and lah_row of series and interval_series (gft[i]_series_observe_negbinomial,
gft[i]_series2_observe_negbinomial, gft[i]_series_lah_row).

Every coefficient of every item carries the oracle's bits -- the reference's own sequence (generating_function.rs:731-750) replayed
per item through OTP / OTPI -- on data without exact zeros: both sides of the form switch at degree_p1 + order = 64, every layout of
a, x, p and ls, out=, the forms against each other, the limits.  Where the reference's Mul looks at the data (exact zeros, a zero
entry of the row, p of 0) and for non-finite values the yardstick is the numpy model of tests/_series_observe_negbinomial_model.py,
itself held to the oracle by the CPU tests."""
import ctypes as C

import numpy as np
import pytest

import _series_observe_model as M
import _series_observe_negbinomial_model as NM
from _series2_oracle import assert_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
LENGTHS = [(6,), (9,), (33,), (64,), (65,), (130,)]
SHAPES = [(5, 7), (7, 5), (1, 9), (9, 1), (3, 66), (66, 3), (12, 12)]
BATCH = (3, 2)
XS = np.array([[0.3, -1.7], [1.0, 0.0], [-0.0, 2.5]])  # per item: ordinary values, one, both zeros
PS = np.array([[0.25, 0.5], [0.9, 1.0], [1.0, 0.75]])  # per item; 1.0 by value returns var itself


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
    """uniform in [-0.5, 0.5) without exact zeros; intervals [v, v + w] with 0 < w < 1e-3 |v| that do not reach zero"""
    rng = np.random.default_rng(seed)
    v = rng.random(shape) - 0.5
    v[v == 0.0] = 0.25
    if not interval:
        return v
    hi = v + rng.random(shape) * 1e-3 * np.abs(v) + 1e-12 * np.abs(v)
    return np.stack([v, hi])


def scalars(xs, interval):
    """the scalars x or p: points at 0, -0 and 1, a width on the others"""
    xs = np.asarray(xs, dtype=np.float64)
    if not interval:
        return xs
    plain = (xs != 0.0) & (xs != 1.0)
    return np.stack([xs, np.where(plain, xs + 1e-3 * np.abs(xs), xs)])


def rows(shape, seed, interval):
    """a dense row in [0.25, 1.25) with a 1.0 at entry 0 of every other item and in the middle of the row of the first"""
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


def grid(length):
    """(K, degree_p1): K in {0, 1, 2, 5, L - 3}, degree_p1 in {3, 4, L - K}, where the shape rules admit them"""
    return [(k, d) for k in sorted({0, 1, 2, 5, length - 3}) for d in sorted({3, 4, length - k}) if k >= 0 and d >= 3 and d + k <= length]


def call(mod, a, var, x, p, ls, d, rank, **kw):
    return mod.observe_negbinomial(a, *(() if rank == 1 else (var,)), x, p, ls, d, **kw)


def layouts(seed, item, n, interval):
    """(a, x, p, ls) four ways over the batch [3, 2]: contiguous; stride 0 (a over batch axis 0, x over axis 1, p over axis 0, ls over
    axis 0, left to the call's own broadcast); sliced from wider tensors; transposed batch axes"""
    lead = (2,) if interval else ()
    q = len(lead)
    wide = item[:-1] + (item[-1] + 3,)
    t = lambda v: dev(v).transpose(q, q + 1)  # noqa: E731
    out = {
        "contiguous": (dev(values(BATCH + item, seed, interval)), dev(scalars(XS, interval)), dev(scalars(PS, interval)),
                       dev(rows(BATCH + (n,), seed + 1, interval))),
        "stride 0": (dev(values((1, BATCH[1]) + item, seed + 2, interval)).expand(lead + BATCH + item), dev(scalars(XS[:, :1], interval)),
                     dev(scalars(PS[:1], interval)), dev(rows((BATCH[1], n), seed + 3, interval))),
        "sliced": (dev(values(BATCH + wide, seed + 4, interval))[..., 1:1 + item[-1]], dev(scalars(np.repeat(XS, 2, axis=1), interval))[..., ::2],
                   dev(scalars(np.repeat(PS, 3, axis=1), interval))[..., 1::3], dev(rows(BATCH + (n + 3,), seed + 5, interval))[..., 1:1 + n]),
        "transposed": (t(values((BATCH[1], BATCH[0]) + item, seed + 6, interval)), t(scalars(XS.T, interval)), t(scalars(PS.T, interval)),
                       dev(rows((BATCH[1], BATCH[0], n), seed + 7, interval)).transpose(q, q + 1)),
    }
    a, x, p, ls = out["stride 0"]
    assert a.stride(q) == 0 and x.shape[-1] == 1 and p.shape[q] == 1 and ls.dim() == q + 2
    assert out["sliced"][1].stride(-1) == 2 and out["sliced"][2].stride(-1) == 3 and not out["transposed"][0].is_contiguous()
    return out


def expected(T, a, item, var, x, p, ls, d, interval):
    """the oracle's sequence per item on the host copies"""
    return NM.oracle_negbinomial(T, a.cpu().numpy(), item, var, x.cpu().numpy(), p.cpu().numpy(), ls.cpu().numpy(), d, interval)


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("item", LENGTHS + SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_exact_against_the_oracle(item, interval, OTP, OTPI):
    from genfer_amd import series

    rank = len(item)
    mod, T = module(rank, interval), OTPI if interval else OTP
    checked = 0
    for var in ((0,) if rank == 1 else (0, 1)):
        L = item[var]
        for k, d in grid(L):
            want_form = "A" if d + k <= 64 else "B"
            for name, (a, x, p, ls) in layouts(1000 * item[0] + 10 * item[-1] + k, item, k + 1, interval).items():
                got = call(mod, a, var, x, p, ls, d, rank)
                assert series.last_form() == want_form
                want = expected(T, a, item, var, x, p, ls, d, interval)
                assert_bits(got, want, f"{item} var={var} K={k} degree_p1={d} {name}")
                checked += 1
                if name == "sliced" and want_form == "A":  # form B on the same call
                    series.set_form("B")
                    try:
                        got = call(mod, a, var, x, p, ls, d, rank)
                        assert series.last_form() == "B"
                    finally:
                        series.set_form(None)
                    assert_bits(got, want, f"{item} var={var} K={k} degree_p1={d} {name} form B")
            # degree_p1 defaults to L - K
            a, x, p, ls = layouts(7, item, k + 1, interval)["contiguous"]
            assert call(mod, a, var, x, p, ls, None, rank).shape[-rank:] == NM.result_shape(item, var, L - k)
    assert checked >= 4 or min(item) == 1


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_out_views_and_overlaps(interval, OTP, OTPI):
    """out= into a strided view with the guard around it untouched; a result inside a, x, p or ls is refused, and torch's next
    operation succeeds behind each refusal"""
    from genfer_amd.taylor import TaylorError

    T, lead = (OTPI if interval else OTP), ((2,) if interval else ())
    for item, var, k, d in (((9,), 0, 2, 5), ((5, 7), 1, 3, 4), ((7, 5), 0, 2, 3), ((66, 3), 0, 5, 61)):
        rank = len(item)
        mod = module(rank, interval)
        a, x, p, ls = layouts(50 + rank, item, k + 1, interval)["contiguous"]
        res = NM.result_shape(item, var, d)
        buf = torch.full(lead + (BATCH[0], 2 * BATCH[1]) + res[:-1] + (res[-1] + 2,), -7.0, dtype=torch.float64, device=DEV)
        view = buf[..., ::2, :, 1:1 + res[-1]] if rank == 2 else buf[..., ::2, 1:1 + res[-1]]
        assert call(mod, a, var, x, p, ls, d, rank, out=view) is view
        assert_bits(view, expected(T, a, item, var, x, p, ls, d, interval), f"{item} out=view")
        mask = torch.ones_like(buf, dtype=torch.bool)
        (mask[..., ::2, :, 1:1 + res[-1]] if rank == 2 else mask[..., ::2, 1:1 + res[-1]]).fill_(False)
        assert (buf[mask] == -7.0).all()
        n_out = int(np.prod(lead + BATCH + res))
        for who, t in (("a", a), ("x", x), ("p", p), ("ls", ls)):
            flat = torch.zeros(t.numel() + n_out + 8, dtype=torch.float64, device=DEV)
            inside = flat[:t.numel()].view(t.shape).copy_(t)
            args = {"a": a, "x": x, "p": p, "ls": ls, who: inside}
            with pytest.raises(TaylorError, match=f"partially overlaps {who}"):
                call(mod, args["a"], var, args["x"], args["p"], args["ls"], d, rank, out=flat[1:1 + n_out].view(lead + BATCH + res))
            assert float((flat[:4] + 1.0).sum().item()) == float((inside.reshape(-1)[:4] + 1.0).sum().item())


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_the_two_forms_give_the_same_bits(interval):
    """series_form 1 and 2 on lines of degree_p1 + order <= 64: identical bits; gft_series_last_form() reports the form; beyond 64
    form A falls back to form B"""
    from genfer_amd import series

    try:
        for item, var, k, d in (((9,), 0, 5, 3), ((64,), 0, 60, 4), ((33,), 0, 2, 31), ((64,), 0, 31, 33), ((5, 7), 1, 2, 5), ((12, 12), 0, 5, 7),
                                ((3, 66), 0, 0, 3)):
            rank = len(item)
            mod = module(rank, interval)
            a, x, p, ls = layouts(80 + rank, item, k + 1, interval)["sliced"]
            got = {}
            for form in ("A", "B"):
                series.set_form(form)
                got[form] = call(mod, a, var, x, p, ls, d, rank)
                assert series.last_form() == form
            assert torch.equal(got["A"].view(torch.int64), got["B"].view(torch.int64)), (item, var, k, d)
        series.set_form("A")
        a, x, p, ls = layouts(90, (65,), 3, interval)["contiguous"]
        call(module(1, interval), a, 0, x, p, ls, 63, 1)
        assert series.last_form() == "B"
    finally:
        series.set_form(None)


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_against_the_model_where_the_oracle_is_no_yardstick(interval):
    """data with +-0, inf and NaN, entries of the row of 0, -0, 1 and non-finite ones, p of 0, 1 and non-finite scalars, x of both
    zeros: the stated loops, bit for bit, in both forms' ranges"""
    A = M.IV if interval else M.F64
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0])
    for item, var, k, d in (((12,), 0, 4, 3), ((70,), 0, 5, 9), ((6, 9), 1, 3, 4), ((9, 6), 0, 3, 4), ((2, 70), 1, 4, 60)):
        rank = len(item)
        mod = module(rank, interval)
        rng = np.random.default_rng(5 + item[0])
        a = rng.random((8,) + item) - 0.5
        pick = rng.random(a.shape) < 0.3
        a[pick] = rng.choice(special, size=int(pick.sum()))
        x = np.array([0.3, 0.0, -0.0, 1.0, np.inf, np.nan, -2.0, 0.5])
        p = np.array([0.5, 0.25, 1.0, 0.0, 0.9, 0.75, np.inf, np.nan])
        ls = 0.25 + rng.random((8, k + 1))
        ls[0, 0] = 0.0            # the sum starts as the zero
        ls[1, k] = -0.0           # -0.0 counts as zero, in the last pass too
        ls[2, 0] = np.inf
        ls[3, 1] = np.nan
        ls[4, :] = 0.0            # every entry zero: the item is all +0.0
        ls[5, k // 2] = 1.0
        ls[6, 1] = -1.0
        if interval:
            a, x, p, ls = np.stack([a, a]), np.stack([x, x]), np.stack([p, p]), np.stack([ls, ls])
            a[1, 7], ls[1, 7] = a[0, 7] + 0.25, ls[0, 7] * 1.5  # one item of wide intervals
        axis = -1 if rank == 1 else var - 2
        got = call(mod, dev(a), var, dev(x), dev(p), dev(ls), d, rank)
        want = NM.observe_negbinomial(A, a, axis, x, p, ls, d, rank)
        assert_bits(got, want, f"{item} var={var}")
        g = got.cpu().numpy()
        zero = g[:, 4] if interval else g[4]
        assert (zero == 0.0).all() and not np.signbit(zero).any()


def test_point_intervals_through_plane_stride_0(OTPI):
    """a.expand(2, ...), x, p and ls likewise are point intervals: plane stride 0, no copy"""
    for item, var, k, d in (((9,), 0, 2, 7), ((5, 7), 1, 3, 3), ((66, 3), 0, 4, 62)):
        rank = len(item)
        mod = module(rank, True)
        a, x, p, ls = (t.expand((2,) + tuple(t.shape)) for t in layouts(60 + rank, item, k + 1, False)["contiguous"])
        assert a.stride(0) == 0 and x.stride(0) == 0 and p.stride(0) == 0 and ls.stride(0) == 0
        assert_bits(call(mod, a, var, x, p, ls, d, rank), expected(OTPI, a, item, var, x, p, ls, d, True), f"{item} var={var}")


def test_the_limits(OTP, OTPI):
    """3 items of the longest line the operation's own limit admits with K = 8 (3 * degree_p1 + K <= 8192, intervals 4096) and of the
    largest rank-2 items carry the oracle's bits; one coefficient more is refused"""
    from genfer_amd import interval_series, interval_series2, series, series2
    from genfer_amd.taylor import TaylorError

    x3, p3 = np.array([0.3, 0.0, 1.0]), np.array([0.25, 0.9, 1.0])
    a, x, p, ls = dev(values((3, 2736), 5, False)), dev(x3), dev(p3), dev(rows((3, 9), 6, False))
    assert_bits(series.observe_negbinomial(a, x, p, ls), expected(OTP, a, (2736,), 0, x, p, ls, 2728, False), "2736, K = 8")
    a, ls = dev(values((3, 64, 64), 7, False)), dev(rows((3, 9), 8, False))
    for var in (0, 1):
        assert_bits(series2.observe_negbinomial(a, var, x, p, ls), expected(OTP, a, (64, 64), var, x, p, ls, 56, False), f"64x64 var={var}, K = 8")
    a, x, p, ls = dev(values((3, 1370), 9, True)), dev(scalars(x3, True)), dev(scalars(p3, True)), dev(rows((3, 9), 10, True))
    assert_bits(interval_series.observe_negbinomial(a, x, p, ls), expected(OTPI, a, (1370,), 0, x, p, ls, 1362, True), "interval 1370, K = 8")
    a, ls = dev(values((3, 32, 64), 11, True)), dev(rows((3, 9), 12, True))
    assert_bits(interval_series2.observe_negbinomial(a, 1, x, p, ls), expected(OTPI, a, (32, 64), 1, x, p, ls, 56, True), "interval 32x64, K = 8")
    ones = lambda *s: torch.ones(s, dtype=torch.float64, device=DEV)  # noqa: E731
    with pytest.raises(TaylorError, match=r"3 \* degree_p1 \+ order = 3 \* 2729 \+ 8 exceeds the limit of 8192"):
        series.observe_negbinomial(ones(1, 2737), ones(1), ones(1), ones(1, 9))
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series.observe_negbinomial(ones(1, 4097), ones(1), ones(1), ones(1, 2))
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series2.observe_negbinomial(ones(1, 64, 65), 1, ones(1), ones(1), ones(1, 2))
    with pytest.raises(TaylorError, match=r"3 \* 1363 \+ 8 exceeds the limit of 4096"):
        interval_series.observe_negbinomial(ones(2, 1, 1371), ones(2, 1), ones(2, 1), ones(2, 1, 9))


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_seventy_thousand_items(interval):
    """more lines than the launches have places for, so both kernels stride over them: 70 000 items of L = 8, K = 2, degree_p1 = 4
    (form B caps at 65 536 workgroups) and of (4, 8) with four lines each (form A caps at 262 144 waves), against the vectorised model"""
    from genfer_amd import series

    A = M.IV if interval else M.F64
    B = 70000
    try:
        for item, var in (((8,), 0), ((4, 8), 1)):
            rank = len(item)
            mod = module(rank, interval)
            a = values((B,) + item, 70 + rank, interval)
            x = scalars(np.resize(XS.reshape(-1), B), interval)
            p = scalars(np.resize(np.array([0.25, 0.5, 0.9, 1.0, 0.75]), B), interval)
            ls = rows((B, 3), 71, interval)
            want = NM.observe_negbinomial(A, a, -1, x, p, ls, 4, rank)
            for form in ("A", "B"):
                series.set_form(form)
                assert_bits(call(mod, dev(a), var, dev(x), dev(p), dev(ls), 4, rank), want, f"{item} form {form}")
    finally:
        series.set_form(None)


def test_a_side_stream(OTP):
    """the call is ordered on torch's current stream: operands produced on a side stream, the result consumed there"""
    from genfer_amd import series

    a, x, p, ls = layouts(33, (33,), 6, False)["contiguous"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a2 = a * 2.0
        got = series.observe_negbinomial(a2, x, p, ls, 20)
        twice = got + got
    s.synchronize()
    want = expected(OTP, a2, (33,), 0, x, p, ls, 20, False)
    assert_bits(got, want, "side stream")
    assert torch.equal(twice, got + got)


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("order", [0, 1, 2, 7, 63, 64, 130])
def test_lah_row(order, interval, OTP, OTPI):
    """257 items of p in {0.25, 0.9, 1.0} (intervals: a width on the first two), contiguous, strided and broadcast, against the model
    on every item and against the oracle's scalars on the three distinct ones; both forms up to 64 entries"""
    from genfer_amd import series

    mod, A, T = module(1, interval), (M.IV if interval else M.F64), (OTPI if interval else OTP)
    base = np.array([0.25, 0.9, 1.0])
    pn = scalars(np.resize(base, 257), interval)
    want = NM.lah_row(A, pn, order)
    three = NM.oracle_lah_row(T, pn[..., :3], order, interval)
    assert_bits(torch.from_numpy(np.ascontiguousarray(want[..., :3, :])), three, f"order {order}: the model against the oracle")
    got = mod.lah_row(dev(pn), order)
    assert series.last_form() == ("A" if order + 1 <= 64 else "B")
    assert got.shape[-2:] == (257, order + 1)
    assert_bits(got, want, f"order {order}")
    wide = dev(scalars(np.repeat(np.resize(base, 257), 2), interval))[..., ::2]
    assert wide.stride(-1) == 2
    assert_bits(mod.lah_row(wide, order), want, f"order {order} strided p")
    one = dev(scalars(base[:1], interval)).expand(((2,) if interval else ()) + (257,))
    assert one.stride(-1) == 0
    assert_bits(mod.lah_row(one, order), np.broadcast_to(want[..., :1, :], want.shape), f"order {order} broadcast p")
    out = torch.full(((2,) if interval else ()) + (257, order + 3), -7.0, dtype=torch.float64, device=DEV)
    view = out[..., 1:order + 2]
    assert mod.lah_row(dev(pn), order, out=view) is view
    assert_bits(view, want, f"order {order} out=view")
    assert (out[..., 0] == -7.0).all() and (out[..., -1] == -7.0).all()
    if order + 1 <= 64:
        series.set_form("B")
        try:
            assert_bits(mod.lah_row(dev(pn), order), want, f"order {order} form B")
            assert series.last_form() == "B"
        finally:
            series.set_form(None)


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_round_trip_with_the_lah_row(interval, OTP, OTPI):
    """observe_negbinomial(..., lah_row(p, K), ...) against the oracle's sequence fed the oracle's own row; p == 1 makes every entry
    past the first zero, where the model is the yardstick"""
    T, A = (OTPI, M.IV) if interval else (OTP, M.F64)
    pn = scalars(np.array([[0.25, 0.5], [0.9, 0.75], [0.1, 0.6]]), interval)
    for item, var, k, d in (((9,), 0, 2, 7), ((33,), 0, 5, 20), ((130,), 0, 7, 100), ((7, 5), 0, 3, 4), ((5, 7), 1, 2, 5)):
        rank = len(item)
        mod, rowmod = module(rank, interval), module(1, interval)
        a, x, _, _ = layouts(40 + rank, item, k + 1, interval)["contiguous"]
        p = dev(pn)
        ls = rowmod.lah_row(p, k)
        assert_bits(ls, NM.oracle_lah_row(T, pn, k, interval), f"{item} K={k}: the row")
        got = call(mod, a, var, x, p, ls, d, rank)
        assert_bits(got, expected(T, a, item, var, x, p, ls, d, interval), f"{item} var={var} K={k}")
        ones = torch.ones_like(p)
        axis = -1 if rank == 1 else var - 2
        got = call(mod, a, var, x, ones, rowmod.lah_row(ones, k), d, rank)
        want = NM.observe_negbinomial(A, a.cpu().numpy(), axis, x.cpu().numpy(), np.ones(pn.shape), NM.lah_row(A, np.ones(pn.shape), k), d, rank)
        assert_bits(got, want, f"{item} var={var} K={k} p == 1")


def test_the_library_refuses_by_itself():
    """the C entry points judge the row, degree_p1 and the result's shape themselves, by name, and write nothing"""
    from genfer_amd import series

    L = series._lib()
    a = torch.ones((2, 9), dtype=torch.float64, device=DEV)
    x, pv, ls = (torch.ones(s, dtype=torch.float64, device=DEV) for s in ((2,), (2,), (2, 3)))
    out = torch.full((2, 9), -7.0, dtype=torch.float64, device=DEV)
    bsz, rbs = (C.c_size_t * 1)(2), (C.c_int64 * 1)(9)  # the result's items lie 9 apart
    q = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = lambda n, d, m: (q(a), None, 9, q(x), None, q(pv), None, q(ls), None, n, d, q(out), rbs, m, bsz, 1, None)  # noqa: E731
    for (n, d, m), text in (((3, 2, 2), "degree_p1 = 2"), ((0, 3, 3), "ls holds no entry"), ((3, 8, 8), "degree_p1 + order = 8 + 2, but a has 9"),
                            ((3, 6, 5), "the result has 5 coefficients; with degree_p1 = 6 it has 6")):
        assert L.gft_series_observe_negbinomial(*args(n, d, m)) != 0
        assert text in L.gft_last_error().decode(), L.gft_last_error().decode()
    assert L.gft_series2_observe_negbinomial(q(a), None, 9, 1, 9, 2, q(x), None, q(pv), None, q(ls), None, 3, 6, q(out), None, 6, 1, 6, bsz, 1,
                                             None) != 0
    assert "var = 2" in L.gft_last_error().decode()
    assert L.gft_series_lah_row(q(pv), None, 4096, q(out), rbs, bsz, 1, None) != 0
    assert "order + 1 = 4097 exceeds the limit of 4096" in L.gft_last_error().decode()
    assert L.gft_series_lah_row(q(out), None, 2, q(out), rbs, bsz, 1, None) != 0
    assert "partially overlaps p" in L.gft_last_error().decode()
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert L.gft_series_observe_negbinomial(*args(3, 6, 6)) == 0  # and the same call within the rules runs
    torch.cuda.synchronize()
    assert (out[:, :6] != -7.0).all() and (out[:, 6:] == -7.0).all()
