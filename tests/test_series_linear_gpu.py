"""The batched affine substitutions on the MI355X: mul_linear and compose_linear of genfer_amd.series, series2, interval_series,
interval_series2 (gft[i]_series[2]_mul_linear / _compose_linear).

Every coefficient of every item carries the oracle's bits (OTP / OTPI per item: mul_linear, and subst_var with the affine series
[c, m] on axis wvar) on data without exact zeros, the stored shape is the definition's compact shape and everything of n outside it is
+0.0: both sides of the form switch at 64 coefficients, every (var, wvar), every layout of the operand and the scalars, out=, the
forms against each other, the limits.  For exact zeros and non-finite values the yardstick is the numpy model of
tests/_series_linear_model.py, itself held to the oracle by the CPU tests."""
import ctypes as C

import numpy as np
import pytest

import _series_linear_model as LM
import _series_observe_model as M
from _series2_oracle import assert_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
ORDERS = [2, 3, 9, 33, 64, 65, 130]
SHAPES = [(5, 7), (7, 5), (1, 9), (9, 1), (3, 66), (66, 3), (12, 12)]
BATCH = (3, 2)
CS = np.array([[0.0, -0.0], [1.0, 0.3], [-1.7, 2.5]])  # per item: both zeros (the power table / mul_var alone), one, ordinary values
MS = np.array([[1.7, 0.5], [1.0, -0.4], [0.9, 1.0]])


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd
    from genfer_amd import series

    genfer_amd.init(0)
    yield
    series.set_form(None)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).reshape(np.shape(a)).to(DEV)  # (ascontiguousarray makes a scalar one-dimensional)


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
    """the scalars c or m: points at 0, -0 and 1, a width on the others"""
    xs = np.asarray(xs, dtype=np.float64)
    if not interval:
        return xs
    plain = (xs != 0.0) & (xs != 1.0)
    return np.stack([xs, np.where(plain, xs + 1e-3, xs)])


def call(mod, op, a, v, w, c, m, n, rank, **kw):
    if op == "mul_linear":
        return mod.mul_linear(a, *(() if rank == 1 else (w,)), c, m, n=n if n is None or rank == 2 else n[0], **kw)
    if rank == 1:
        return mod.compose_linear(a, c, m, n=None if n is None else n[0], **kw)
    return mod.compose_linear(a, v, c, m, wvar=w, n=n, **kw)


def layouts(seed, item, interval):
    """(a, c, m) four ways over the batch [3, 2]: contiguous; strided rows with scalars sliced out of wider tensors; stride 0 (the
    operand over batch axis 0, c over axis 1, m one value for all, left to the call's own broadcast); transposed batch axes"""
    lead = (2,) if interval else ()
    p = len(lead)
    wide = item[:-1] + (item[-1] + 3,)
    t = lambda x: dev(x).transpose(p, p + 1)  # noqa: E731
    out = {
        "contiguous": (dev(values(BATCH + item, seed, interval)), dev(scalars(CS, interval)), dev(scalars(MS, interval))),
        "strided rows": (dev(values(BATCH + wide, seed + 4, interval))[..., 1:1 + item[-1]], dev(scalars(np.repeat(CS, 2, axis=1), interval))[..., ::2],
                         dev(scalars(np.repeat(MS, 3, axis=1), interval))[..., 1::3]),
        "stride 0": (dev(values((1, BATCH[1]) + item, seed + 2, interval)).expand(lead + BATCH + item), dev(scalars(CS[:, :1], interval)),
                     dev(scalars(MS[1, 1], interval))),
        "transposed": (t(values((BATCH[1], BATCH[0]) + item, seed + 6, interval)), t(scalars(CS.T, interval)), t(scalars(MS.T, interval))),
    }
    a, c, m = out["stride 0"]
    assert a.stride(p) == 0 and c.shape[-1] == 1 and m.dim() == p
    assert out["strided rows"][1].stride(-1) == 2 and out["strided rows"][2].stride(-1) == 3 and not out["transposed"][0].is_contiguous()
    return out


def expected(T, op, a, item, v, w, c, m, n, interval):
    """the oracle per item on the host copies, inside +0.0 at the orders n"""
    A = M.IV if interval else M.F64
    want = LM.oracle_linear(T, op, a.cpu().numpy(), item, v, w, c.cpu().numpy(), m.cpu().numpy(), n, interval)
    return LM.padded(A, want, n, len(item))


def assert_result(got, want, what):
    assert tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    assert_bits(got, want, what)  # (bit for bit: the padding is +0.0, not -0.0)


def orders2(item, v, w, limit):
    """the orders of a rank-2 case: the least ones (two on w: truncating where w != v), and room around the untruncated shape -- two
    more on w, one more line -- as far as the limit lets it"""
    o = 1 - w
    least = tuple(max(k, 2) if i == w else k for i, k in enumerate(item))
    lines = item[o] + 1 if (item[o] + 1) * max(item[w], 2) <= limit else item[o]
    room = [0, 0]
    room[o], room[w] = lines, max(min(LM.default_order("compose_linear", item, v, w)[w] + 2, limit // lines), item[w], 2)
    return [least, tuple(room)]


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("n", ORDERS)
def test_rank1_bit_exact_against_the_oracle(n, interval, OTP, OTPI):
    from genfer_amd import series

    mod, T = module(1, interval), OTPI if interval else OTP
    for nf in sorted({1, 2, 3, n}):
        if nf > n:
            continue
        for name, (a, c, m) in layouts(100 * n + nf, (nf,), interval).items():
            got = call(mod, "compose_linear", a, 0, 0, c, m, (n,), 1)
            assert series.last_form() == ("A" if n <= 64 else "B")
            assert_result(got, expected(T, "compose_linear", a, (nf,), 0, 0, c, m, (n,), interval), f"compose_linear nf={nf} n={n} {name}")
        if nf < n:  # n above L; n == L is the next one's
            got = call(mod, "mul_linear", a, 0, 0, c, m, (n,), 1)
            assert_result(got, expected(T, "mul_linear", a, (nf,), 0, 0, c, m, (n,), interval), f"mul_linear L={nf} n={n}")
    a, c, m = layouts(7 + n, (n,), interval)["strided rows"]
    assert_result(call(mod, "mul_linear", a, 0, 0, c, m, (n,), 1), expected(T, "mul_linear", a, (n,), 0, 0, c, m, (n,), interval), f"mul_linear L=n={n}")
    assert series.last_form() is None  # (one streaming kernel)
    # the default orders: f's stored length; one more than a's
    assert call(mod, "compose_linear", a, 0, 0, c, m, None, 1).shape[-1] == n
    assert call(mod, "mul_linear", a, 0, 0, c, m, None, 1).shape[-1] == n + 1


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("item", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rank2_bit_exact_against_the_oracle(item, interval, OTP, OTPI):
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    mod, T = module(2, interval), OTPI if interval else OTP
    checked = 0
    for v in (0, 1):
        for w in (0, 1):
            for n in orders2(item, v, w, 2048 if interval else 4096):
                for name, (a, c, m) in layouts(1000 * item[0] + 10 * item[1] + 2 * v + w, item, interval).items():
                    got = call(mod, "compose_linear", a, v, w, c, m, n, 2)
                    assert series.last_form() == ("A" if n[w] <= 64 else "B")
                    assert_result(got, expected(T, "compose_linear", a, item, v, w, c, m, n, interval), f"compose_linear {item} v={v} w={w} n={n} {name}")
                    checked += 1
                if v == w:
                    got = call(mod, "mul_linear", a, v, w, c, m, n, 2)
                    assert_result(got, expected(T, "mul_linear", a, item, v, w, c, m, n, interval), f"mul_linear {item} w={w} n={n}")
            a, c, m = layouts(3, item, interval)["contiguous"]
            dn = LM.default_order("compose_linear", item, v, w)  # the default orders: the stored shape, f's own length on var
            if dn[w] >= 2 and dn[0] * dn[1] <= (2048 if interval else 4096):
                assert tuple(call(mod, "compose_linear", a, v, w, c, m, None, 2).shape[-2:]) == dn
            elif dn[w] >= 2:
                with pytest.raises(TaylorError, match="exceeds the limit"):
                    call(mod, "compose_linear", a, v, w, c, m, None, 2)
        assert tuple(mod.mul_linear(a, v, c, m).shape[-2:]) == LM.default_order("mul_linear", item, v, v)
        # wvar defaults to var
        if item[v] >= 2:
            u, z = mod.compose_linear(a, v, c, m), mod.compose_linear(a, v, c, m, wvar=v)
            assert torch.equal(u.view(torch.int64), z.view(torch.int64))
    assert checked >= 32


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_out_views_and_overlaps(interval, OTP, OTPI):
    """out= into a strided view with the guard around it untouched; a result that touches the operand, c or m is refused, the operand's
    own view included"""
    from genfer_amd.taylor import TaylorError

    T, lead = (OTPI if interval else OTP), ((2,) if interval else ())
    for op, item, v, w, n in (("compose_linear", (9,), 0, 0, (12,)), ("compose_linear", (5, 7), 1, 1, (6, 9)), ("compose_linear", (7, 5), 0, 1, (7, 11)),
                              ("compose_linear", (66, 3), 0, 0, (70, 4)), ("mul_linear", (9,), 0, 0, (10,)), ("mul_linear", (5, 7), 0, 0, (6, 8))):
        rank = len(item)
        mod = module(rank, interval)
        a, c, m = layouts(50 + rank, item, interval)["contiguous"]
        buf = torch.full(lead + (BATCH[0], 2 * BATCH[1]) + n[:-1] + (n[-1] + 2,), -7.0, dtype=torch.float64, device=DEV)
        view = buf[..., ::2, :, 1:1 + n[-1]] if rank == 2 else buf[..., ::2, 1:1 + n[-1]]
        assert call(mod, op, a, v, w, c, m, None, rank, out=view) is view  # (the orders are out's)
        assert_result(view, expected(T, op, a, item, v, w, c, m, n, interval), f"{op} {item} out=view")
        mask = torch.ones_like(buf, dtype=torch.bool)
        (mask[..., ::2, :, 1:1 + n[-1]] if rank == 2 else mask[..., ::2, 1:1 + n[-1]]).fill_(False)
        assert (buf[mask] == -7.0).all()
        n_out = int(np.prod(lead + BATCH + n))
        names = {"a": "f" if op == "compose_linear" else "a", "c": "c", "m": "m"}
        for who, t in (("a", a), ("c", c), ("m", m)):
            flat = torch.zeros(t.numel() + n_out + 8, dtype=torch.float64, device=DEV)
            inside = flat[:t.numel()].view(t.shape).copy_(t)
            args = {"a": a, "c": c, "m": m, who: inside}
            with pytest.raises(TaylorError, match=f"partially overlaps {names[who]}"):
                call(mod, op, args["a"], v, w, args["c"], args["m"], n, rank, out=flat[1:1 + n_out].view(lead + BATCH + n))
    # in place is refused: the result is no operand
    a, c, m = layouts(9, (9,), interval)["contiguous"]
    with pytest.raises(TaylorError, match="partially overlaps f"):
        module(1, interval).compose_linear(a, c, m, out=a)


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_the_two_forms_give_the_same_bits(interval):
    """series_form 1 and 2 on lines of at most 64 coefficients: identical bits; gft_series_last_form() reports the form; beyond 64
    form A falls back to form B"""
    from genfer_amd import series

    try:
        for item, v, w, n in (((33,), 0, 0, (33,)), ((64,), 0, 0, (64,)), ((3,), 0, 0, (64,)), ((5, 7), 1, 1, (6, 9)), ((12, 12), 0, 1, (12, 23)),
                              ((12, 12), 1, 0, (20, 12)), ((33, 2), 0, 0, (33, 3))):
            rank = len(item)
            mod = module(rank, interval)
            a, c, m = layouts(80 + rank, item, interval)["strided rows"]
            got = {}
            for form in ("A", "B"):
                series.set_form(form)
                got[form] = call(mod, "compose_linear", a, v, w, c, m, n, rank)
                assert series.last_form() == form
            assert torch.equal(got["A"].view(torch.int64), got["B"].view(torch.int64)), (item, v, w, n)
        series.set_form("A")
        a, c, m = layouts(90, (65,), interval)["contiguous"]
        call(module(1, interval), "compose_linear", a, 0, 0, c, m, (65,), 1)
        assert series.last_form() == "B"
    finally:
        series.set_form(None)


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_against_the_model_where_the_oracle_is_no_yardstick(interval):
    """data with +-0, inf and NaN, zero, -0.0 and non-finite scalars: the stated loops, bit for bit, in both forms' ranges"""
    A = M.IV if interval else M.F64
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0])
    for item, v, w, n in (((12,), 0, 0, (14,)), ((70,), 0, 0, (70,)), ((6, 9), 1, 1, (7, 9)), ((9, 6), 0, 1, (9, 12)), ((2, 70), 0, 1, (2, 71)),
                          ((6, 9), 1, 0, (12, 9))):
        rank = len(item)
        mod = module(rank, interval)
        rng = np.random.default_rng(5 + item[0])
        a = rng.random((8,) + item) - 0.5
        pick = rng.random(a.shape) < 0.3
        a[pick] = rng.choice(special, size=int(pick.sum()))
        c = np.array([0.3, 0.0, -0.0, 1.0, np.inf, np.nan, -2.0, 0.0])
        m = np.array([0.5, -1.5, 2.0, 1.0, 0.25, 3.0, np.inf, np.nan])
        if interval:
            a, c, m = np.stack([a, a]), np.stack([c, c]), np.stack([m, m])
            a[1, 6], c[1, 6], m[1, 0] = a[0, 6] + 0.25, c[0, 6] + 0.5, m[0, 0] * 1.5  # wide intervals
        got = call(mod, "compose_linear", dev(a), v, w, dev(c), dev(m), n, rank)
        assert_result(got, LM.padded(A, LM.compose_linear(A, a, v, c, m, w, n, rank), n, rank), f"compose_linear {item} v={v} w={w}")
        got = call(mod, "mul_linear", dev(a), v, w, dev(c), dev(m), n, rank)
        assert_result(got, LM.padded(A, LM.mul_linear(A, a, w, c, m, n[w], rank), n, rank), f"mul_linear {item} w={w}")


def test_point_intervals_through_plane_stride_0(OTPI):
    """a.expand(2, ...), c.expand(2, ...) and m.expand(2, ...) are point intervals: plane stride 0, no copy"""
    for op, item, v, w, n in (("compose_linear", (9,), 0, 0, (9,)), ("compose_linear", (5, 7), 1, 0, (11, 7)), ("compose_linear", (66, 3), 0, 0, (66, 3)),
                              ("mul_linear", (5, 7), 1, 1, (5, 8))):
        rank = len(item)
        mod = module(rank, True)
        a, c, m = (t.expand((2,) + tuple(t.shape)) for t in layouts(60 + rank, item, False)["contiguous"])
        assert a.stride(0) == 0 and c.stride(0) == 0 and m.stride(0) == 0
        assert_result(call(mod, op, a, v, w, c, m, n, rank), expected(OTPI, op, a, item, v, w, c, m, n, True), f"{op} {item} v={v} w={w}")


def test_the_limits(OTP, OTPI):
    """n = nf = 4096, 2048 over intervals and (64, 64) run and carry the oracle's bits (one item with c == 0: the power table); one
    coefficient more is refused"""
    from genfer_amd import interval_series, series, series2
    from genfer_amd.taylor import TaylorError

    # (m near 1 and small c keep 4096 Horner steps finite)
    a, c, m = dev(values((2, 4096), 5, False)), dev(np.array([0.01, 0.0])), dev(np.array([0.99, -0.999]))
    assert_result(series.compose_linear(a, c, m), expected(OTP, "compose_linear", a, (4096,), 0, 0, c, m, (4096,), False), "4096")
    assert_result(series.mul_linear(a[:, :4095], c, m), expected(OTP, "mul_linear", a[:, :4095], (4095,), 0, 0, c, m, (4096,), False), "mul_linear 4096")
    a, c, m = dev(values((2, 2048), 9, True)), dev(scalars([0.01, 0.0], True)), dev(scalars([0.99, -0.999], True))
    assert_result(interval_series.compose_linear(a, c, m), expected(OTPI, "compose_linear", a, (2048,), 0, 0, c, m, (2048,), True), "interval 2048")
    a, c, m = dev(values((2, 64, 64), 7, False)), dev(np.array([0.3, 0.0])), dev(np.array([0.7, -0.9]))
    for v, w in ((0, 0), (1, 1), (0, 1), (1, 0)):
        got = series2.compose_linear(a, v, c, m, wvar=w, n=(64, 64))
        assert_result(got, expected(OTP, "compose_linear", a, (64, 64), v, w, c, m, (64, 64), False), f"64x64 v={v} w={w}")
    ones = lambda *s: torch.ones(s, dtype=torch.float64, device=DEV)  # noqa: E731
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series.compose_linear(ones(1, 9), ones(1), ones(1), n=4097)
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series2.mul_linear(ones(1, 64, 64), 1, ones(1), ones(1))
    with pytest.raises(TaylorError, match="exceeds the limit of 2048"):
        interval_series.mul_linear(ones(2, 1, 2048), ones(2, 1), ones(2, 1))


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_seventy_thousand_items(interval):
    """more lines than the launches have places for, so every kernel strides over them: 70 000 items of 8 coefficients (form B caps
    at 65 536 workgroups) and of (4, 8) with four lines each (form A caps at 262 144 waves), against the vectorised model"""
    from genfer_amd import series

    A = M.IV if interval else M.F64
    B = 70000
    try:
        for item, v, w, n in (((8,), 0, 0, (8,)), ((4, 8), 1, 1, (4, 8))):
            rank = len(item)
            mod = module(rank, interval)
            a = values((B,) + item, 70 + rank, interval)
            c, m = scalars(np.resize(CS.reshape(-1), B), interval), scalars(np.resize(MS.reshape(-1)[:5], B), interval)
            want = LM.padded(A, LM.compose_linear(A, a, v, c, m, w, n, rank), n, rank)
            for form in ("A", "B"):
                series.set_form(form)
                assert_result(call(mod, "compose_linear", dev(a), v, w, dev(c), dev(m), n, rank), want, f"{item} form {form}")
            series.set_form(None)
            nm = n[:-1] + (n[-1] + 1,)
            want = LM.padded(A, LM.mul_linear(A, a, w, c, m, nm[w], rank), nm, rank)
            assert_result(call(mod, "mul_linear", dev(a), v, w, dev(c), dev(m), nm, rank), want, f"mul_linear {item}")
    finally:
        series.set_form(None)


def test_the_library_refuses_by_itself():
    """the C entry points judge the axes, the orders and the overlaps themselves, by name, and write nothing"""
    from genfer_amd import series

    L = series._lib()
    a = torch.ones((2, 9), dtype=torch.float64, device=DEV)
    c, m = torch.ones(2, dtype=torch.float64, device=DEV), torch.ones(2, dtype=torch.float64, device=DEV)
    out = torch.full((2, 12), -7.0, dtype=torch.float64, device=DEV)
    bsz, rbs = (C.c_size_t * 1)(2), (C.c_int64 * 1)(12)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = lambda na, n: (p(a), None, na, p(c), None, p(m), None, p(out), rbs, n, bsz, 1, None)  # noqa: E731
    for fn in (L.gft_series_compose_linear, L.gft_series_mul_linear):
        for (na, n), text in (((1, 1), "the result has 1 coefficient"), ((9, 8), "> n = 8 (an operand is longer than the truncation order)"),
                              ((9, 4097), "n = 4097 exceeds the limit of 4096")):
            assert fn(*args(na, n)) != 0
            assert text in L.gft_last_error().decode(), L.gft_last_error().decode()
    assert L.gft_series2_compose_linear(p(a), None, 9, 1, 9, 1, 2, p(c), None, p(m), None, p(out), None, 12, 1, 12, bsz, 1, None) != 0
    assert "wvar = 2" in L.gft_last_error().decode()
    assert L.gft_series2_mul_linear(p(a), None, 9, 1, 9, 2, p(c), None, p(m), None, p(out), None, 12, 1, 12, bsz, 1, None) != 0
    assert "var = 2" in L.gft_last_error().decode()
    assert L.gft_series_compose_linear(p(a), None, 9, p(c), None, p(out), None, p(out), rbs, 12, bsz, 1, None) != 0
    assert "partially overlaps m" in L.gft_last_error().decode()
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert L.gft_series_compose_linear(*args(9, 10)) == 0  # and the same call within the rules runs
    torch.cuda.synchronize()
    assert (out[:, :10] != -7.0).all() and (out[:, 10:] == -7.0).all()
