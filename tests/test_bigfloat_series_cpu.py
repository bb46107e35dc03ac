"""Batched BigFloat series (genfer_amd.bigfloat_series, gftb_series_*) without a GPU: the exported and declared surface (six symbols, no
gftb_width), the torch encode / decode against genfer_amd.bigfloat's, every refusal the Python side makes before it touches the
library, the C layer's new refusals in a stand-alone program (tests/series_bigfloat_args_main.cpp), and the expected values of
tests/test_bigfloat_series_gpu.py -- the data, the cases, the raw BigFloat product of tests/series_bigfloat_oracle.cpp, the oracle's
handle operators and the compose / pow chains over that product, checked here against each other, against the definitions written
out in scalar BigFloat operations, and for sanity (no NaN and no inf in any finite case)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, splitmix64_uniform

SYMBOLS = ("gftb_series_mul", "gftb_series_div", "gftb_series_exp", "gftb_series_log", "gftb_series_compose", "gftb_series_pow")
OPS = ("mul", "div", "exp", "log", "compose", "pow")
INF, NAN = float("inf"), float("nan")

# ---- the oracle ------------------------------------------------------------------------------------------------------------------

_ORCB = {}


def orcb_lib(tmp_root):
    """tests/series_bigfloat_oracle.cpp: tests/bigfloat_oracle.cpp (the orcb_ handle operators and orcb_scalar_op) and the raw product
    orcb_series_mul_raw (built once per session)"""
    if "lib" not in _ORCB:
        so = os.path.join(str(tmp_root), "liborcbs.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so,
                               os.path.join(ROOT, "tests", "series_bigfloat_oracle.cpp")])
        L = C.CDLL(so)
        L.orcb_series_mul_raw.restype = C.c_int
        L.orcb_series_mul_raw.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.orcb_scalar_op.restype = C.c_int
        L.orcb_scalar_op.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _ORCB["lib"] = L
    return _ORCB["lib"]


@pytest.fixture(scope="session")
def orcb(tmp_path_factory):
    return orcb_lib(tmp_path_factory.mktemp("orcbs"))


@pytest.fixture(scope="session")
def OTPB(orcb):
    """Oracle-backed TaylorPoly<BigFloat>"""
    from genfer_amd.taylor import bind

    return bind(orcb, "orcb_")


D2 = C.c_double * 2


def scalar_op(orcb, code, a, b=None):
    """one scalar operation of the oracle's BigFloat on {factor, exponent} pairs (orcb_scalar_op: 0 add, 1 sub, 2 mul, 3 div, 4 neg,
    5 exp, 6 log, 7 normalize)"""
    out, x = D2(), D2(float(a[0]), float(a[1]))
    y = None if b is None else D2(float(b[0]), float(b[1]))
    assert orcb.orcb_scalar_op(code, x, y, out) == 0
    return np.array(out[:])


ZERO = np.array([0.0, 0.0])


def from_u32(orcb, k):
    return scalar_op(orcb, 7, (float(k), 0.0))  # normalize(k, 0): BigFloat::from_u32


# ---- the data ----------------------------------------------------------------------------------------------------------------------
KINDS = ("wide", "tiny", "special")
FINITE = ("wide", "tiny")
LOW = (-1025, -1020)  # the low band of "tiny": a low coefficient times a moderate one lies around the cut-off -1024


def data(kind, B, n, seed, head=None):
    """[2, B, n] BigFloat rows = (factor, exponent).
    "wide": factors of both signs in +-[1, 2), exponents spread over +-3000 -- decoded values leave the f64 range and neighbouring terms
    of a sum differ by more than 1023 in exponent (add's powi cut-off inside a sum).
    "tiny": factors of both signs, exponents in the low band LOW or in [-2, 2], sprinkled with {+0, 0} and with {-0, 0} (what a negation
    leaves): terms with exponent <= -1024 meet zero accumulators -- the tiny-term drop of 0 + b -- and sums of a few terms just above
    -1024 cancel to just below it, where the addition onto the zeroed result of mul_rec drops them.
    "near": factors of both signs, exponents in [-20, 20]: no rule of BigFloat's add fires (the cross-checks against the oracle's own
    operators, whose shortcuts then compute the same values).
    "special": the wide rows, each seeded at a coefficient >= 1 with one of {+inf, e}, {-inf, e}, {NaN, e} (retained exponents e) and
    with a {+0, 0}.
    Coefficient 0 -- what div divides by and exp / log take their seed of -- has a positive factor and, with `head` = (lo, hi), an
    exponent in that range (exp needs a moderate one: its seed is 2^(x0 * log2 e)); by default "wide" keeps its +-3000 there too and
    "tiny" a moderate one."""
    u = splitmix64_uniform(seed, 3 * B * n).reshape(3, B, n)
    f = (1.0 + u[0]) * np.where(u[1] < 0.5, -1.0, 1.0)
    assert np.all(np.abs(f) >= 1.0) and np.all(np.abs(f) < 2.0)
    if kind == "tiny":
        low = u[2] < 0.6
        e = np.where(low, np.floor(LOW[0] + (LOW[1] - LOW[0] + 1) * u[2] / 0.6), np.floor(-2.0 + 5.0 * (u[2] - 0.6) / 0.4))
        pick = (u[1] * 16.0) % 1.0
        f = np.where(pick < 0.10, 0.0, np.where(pick < 0.15, -0.0, f))
        e = np.where(f == 0.0, 0.0, e)
        if head is None:
            head = (-3, 4)
    elif kind == "near":
        e = np.floor(-20.0 + 41.0 * u[2])
    else:
        e = np.floor(-3000.0 + 6001.0 * u[2])
    f[:, 0] = 1.0 + u[0][:, 0]
    if head is None and kind == "near":
        head = (-20, 20)
    e[:, 0] = np.floor(-3000.0 + 6001.0 * u[2][:, 0]) if head is None else np.floor(head[0] + (head[1] - head[0] + 1) * u[2][:, 0])
    if kind == "special" and n >= 2:
        kinds = [(INF, 7.0), (-INF, -2000.0), (NAN, 0.0), (NAN, 1500.0), (INF, 0.0)]
        for b in range(B):
            k = 1 + (b // len(kinds)) % (n - 1)
            f[b, k], e[b, k] = kinds[b % len(kinds)]
            z = 1 + (k + 1 + b) % (n - 1)
            if z != k:
                f[b, z], e[b, z] = 0.0, 0.0
    return np.stack([f, e])


def pad(a, n):
    """[2, len] -> [2, n], {+0, 0} beyond"""
    a = np.asarray(a, dtype=np.float64).reshape(2, -1)
    out = np.zeros((2, n))
    out[:, :a.shape[1]] = a
    return out


def same_bits(a, b):
    """every bit of every factor and exponent; where the oracle's factor is a NaN, a NaN (its exponent is compared exactly)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all(np.where(np.isnan(b), np.isnan(a), a.view(np.int64) == b.view(np.int64))))


# ---- the expected values shared with the GPU tests ---------------------------------------------------------------------------------


def mul_raw(orcb, x, y, n):
    """the raw product on one item: x [2, nx], y [2, ny] -> [2, n]"""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    out = np.zeros((2, n))
    assert orcb.orcb_series_mul_raw(C.c_void_p(x.ctypes.data), x.shape[1], C.c_void_p(y.ctypes.data), y.shape[1], C.c_void_p(out.ctypes.data), n) == 0
    return out


def want_mul(orcb, X, Y, n):
    return np.stack([mul_raw(orcb, X[:, b], Y[:, b], n) for b in range(X.shape[1])], axis=1)


def host_seeds(orcb, op, X):
    """[2, B]: BigFloat::exp / log of coefficient 0 per item (orcb_scalar_op 5 and 6: the host libm's values)"""
    return np.stack([scalar_op(orcb, {"exp": 5, "log": 6}[op], X[:, b, 0]) for b in range(X.shape[1])], axis=1)


def define(orcb, op, x, y, n):
    """div / exp / log of one item written out in scalar BigFloat operations: the loops of mt:1162-1192 (one axis), mt:1271-1283 and
    mt:1319-1333, with no shortcut at any length"""
    s = lambda code, a, b=None: scalar_op(orcb, code, a, b)  # noqa: E731
    nx = x.shape[1]
    r = []
    if op == "div":
        ny = y.shape[1]
        for k in range(n):
            acc = ZERO
            for j in range(max(0, k + 1 - ny), k):
                acc = s(0, acc, s(2, r[j], y[:, k - j]))
            c = s(4, acc)
            if k < nx:
                c = s(0, c, x[:, k])
            r.append(s(3, c, y[:, 0]))
    elif op == "exp":
        r.append(s(5, x[:, 0]))
        for k in range(1, n):
            acc = ZERO
            for j in range(1, min(nx, k + 1)):
                acc = s(0, acc, s(2, s(2, x[:, j], from_u32(orcb, j)), r[k - j]))
            r.append(s(3, acc, from_u32(orcb, k)))
    else:
        r.append(s(6, x[:, 0]))
        for k in range(1, n):
            if nx == 1:
                r.append(ZERO)  # (the reference stores no higher order of a one-coefficient operand)
                continue
            acc = ZERO
            for j in range(max(k + 1 - nx, 1), k):
                acc = s(0, acc, s(2, s(2, x[:, k - j], r[j]), from_u32(orcb, j)))
            xk = x[:, k] if k < nx else ZERO
            r.append(s(3, s(3, s(1, s(2, xk, from_u32(orcb, k)), acc), x[:, 0]), from_u32(orcb, k)))
    return np.array(r).T


def want_handle(orcb, OTPB, op, X, Y, n):
    """div / exp / log through the oracle's handle operators per item where the divisor / the operand holds at least two coefficients,
    so that the operators take their general paths (their shortcuts look at the stored length, mt:1204-1213); a one-coefficient one
    through the written definition"""
    out = []
    for b in range(X.shape[1]):
        if (Y if op == "div" else X).shape[2] < 2:
            out.append(define(orcb, op, X[:, b], None if Y is None else Y[:, b], n))
            continue
        p = OTPB.new(X[:, b], (n,))
        r = p / OTPB.new(Y[:, b], (n,)) if op == "div" else (p.exp() if op == "exp" else p.log())
        out.append(pad(r.array(), n))
    return np.stack(out, axis=1)


def chain_compose(orcb, f, g, n):
    """the definition: Horner over f with the raw product at the compact length of every step and the oracle's scalar add; one
    coefficient of f gives 0 + f"""
    res = scalar_op(orcb, 0, ZERO, f[:, -1]).reshape(2, 1)
    for i in range(f.shape[1] - 2, -1, -1):
        res = mul_raw(orcb, res, g, min(res.shape[1] + g.shape[1] - 1, n))
        res[:, 0] = scalar_op(orcb, 0, res[:, 0], f[:, i])
    return pad(res, n)


def chain_pow(orcb, x, e, n):
    """the definition: square-and-multiply from the unit series {1, 0} without the last squaring, compact lengths"""
    res, base = np.array([[1.0], [0.0]]), np.array(x, dtype=np.float64)
    while e > 0:
        if e & 1:
            res = mul_raw(orcb, res, base, min(res.shape[1] + base.shape[1] - 1, n))
        e >>= 1
        if e > 0:
            base = mul_raw(orcb, base, base, min(2 * base.shape[1] - 1, n))
    return pad(res, n)


def crafted():
    """Operands on which the addition onto the zeroed result decides a coefficient: two terms at exponent -1022 cancel to a residual
    near -1040, which a sum keeps (its accumulator is not zero) and 0 + sum drops.  {"mul": (x, y, n), "compose": (f, g, n)}, each
    [2, len]; coefficient 1 of either result is {0, 0}, and {-1.5, -1039} or {-1.875 ..., -1042} for a kernel that stores the sum."""
    d = 2.0**-20
    return {"mul": (np.array([[1.5, 1.25], [-511.0, -511.0]]), np.array([[1.5, -1.25 * (1 + d)], [-511.0, -511.0]]), 2),
            "compose": (np.array([[1.0, -(1 + d), 1.0], [0.0, -679.0, -340.0]]), np.array([[1.0, 1.5], [-340.0, -340.0]]), 3)}


def want_compose(orcb, F, G, n):
    return np.stack([chain_compose(orcb, F[:, b], G[:, b], n) for b in range(F.shape[1])], axis=1)


def want_pow(orcb, X, e, n):
    return np.stack([chain_pow(orcb, X[:, b], e, n) for b in range(X.shape[1])], axis=1)


# ---- the cases of the bit-exact GPU test ------------------------------------------------------------------------------------------
# the smallest orders at which a form or a dispatch boundary of W = 2 can go wrong (tests/test_interval_series_gpu.py's boundaries):
# form A's waves per workgroup change at 9 | 10 and 19 | 20, the 64 KB budget ends at 31 | 32, the 80 KB one at 39 | 40, 63 | 64 | 65 is
# the staging width and the wave of form B's division, 129 takes more than one pass of everything
ORDERS = [1, 2, 7, 8, 9, 31, 32, 39, 40, 63, 64, 65, 129]
BATCH = (3, 2)
AUTO = [(9, 256), (9, 257)]  # the automatic choice on both sides of 256 items
COMPACT_AT = (9, 40, 65)  # orders that also run compact operands (nx, ny < n)
LONG = (2048, 2)  # mul and div only
POW_E = [0, 1, 2, 5, 11]
COMPOSE_NF = [1, 2, 5]
EXP_HEAD = (-3, 9)  # exponents of coefficient 0 under exp: seeds up to exp(2^10), far outside f64 and far inside BigFloat


def bit_exact_cases(op):
    """(n, B, nx, ny, e, forms): the operand lengths (compose: nf, ng), pow's exponent, the forms to force"""
    for n in ORDERS:
        forms = ("A", "B")
        if op == "compose":
            for nf in COMPOSE_NF:
                if nf <= n:
                    yield n, 6, nf, n, None, forms
            if n in COMPACT_AT:
                yield n, 6, min(5, n // 2), n // 2 + 1, None, forms
        elif op == "pow":
            for e in POW_E:
                yield n, 6, n, 1, e, forms
            if n in COMPACT_AT:
                yield n, 6, max(1, n // 3), 1, 5, forms
        else:
            yield n, 6, n, n, None, forms
            if n in COMPACT_AT:
                yield n, 6, n // 2, n - 1, None, forms
                if op == "mul":
                    yield n, 6, 1, max(2, n // 3), None, forms
                elif op == "div":
                    yield n, 6, 1, 2, None, forms
                else:
                    yield n, 6, 1, 1, None, forms  # a one-coefficient operand: the seed, then zeros
    for n, B in AUTO:
        if op == "compose":
            yield n, B, 2, n, None, (None,)
        elif op == "pow":
            yield n, B, n, 1, 2, (None,)
        else:
            yield n, B, n, n, None, (None,)
    if op in ("mul", "div"):
        yield LONG[0], LONG[1], LONG[0] // 2, 65, None, (None,)
        yield LONG[0], LONG[1], LONG[0], LONG[0], None, (None,)


def operands(op, kind, n, B, nx, ny):
    head = EXP_HEAD if op == "exp" else None
    X = data(kind, B, nx, 1000 * n + B + 31 * nx, head)
    if op in ("mul", "div", "compose"):
        return X, data(kind, B, ny, 2000 * n + B + 7 + 17 * ny)
    return X, None


def expected(orcb, OTPB, op, kind, n, B, nx, ny, e=None):
    """the operands of a case and the oracle's result"""
    X, Y = operands(op, kind, n, B, nx, ny)
    if op == "mul":
        return X, Y, want_mul(orcb, X, Y, n)
    if op == "compose":
        return X, Y, want_compose(orcb, X, Y, n)
    if op == "pow":
        return X, None, want_pow(orcb, X, e, n)
    return X, Y, want_handle(orcb, OTPB, op, X, Y, n)


# ---- the surface -----------------------------------------------------------------------------------------------------------------


def _product_lib():
    import genfer_amd

    if not os.path.exists(genfer_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return genfer_amd.lib()


def test_six_symbols_are_declared_and_exported_and_nothing_else():
    import genfer_amd

    L = _product_lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert hasattr(L, s), s
        assert f"pub fn {s}(" in doc, s
    assert sorted(set(re.findall(r"\b(gftb_[a-z0-9_]+)\s*\(", header))) == sorted(SYMBOLS)
    assert re.search(r"gftb_series_pow\([^)]*uint32_t\s+e\b", header)
    # the handle family stays out: tests/test_bigfloat_cpu.py pins its absence through gftb_width
    assert not hasattr(L, "gftb_width")
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", genfer_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert sorted(t.split()[-1] for t in out.splitlines() if t.split()[-1].startswith("gftb_")) == sorted(SYMBOLS)


def test_argument_lists_come_from_the_one_table():
    """the ctypes declarations of gftb_series_* are built from the rows of _series_call.OPS and equal those of the gfti_ twins, as the
    header's argument lists do"""
    from genfer_amd import _series_call, bigfloat_series

    _product_lib()
    L = _series_call._lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    for suffix in OPS:
        b, i = getattr(L, "gftb_series_" + suffix), getattr(L, "gfti_series_" + suffix)
        assert b.restype is C.c_int and list(b.argtypes) == list(i.argtypes), suffix
        args = {p: re.sub(r"\s+", " ", re.search(r"\bint\s+" + p + r"series_" + suffix + r"\s*\(([^)]*)\)", header).group(1)) for p in ("gftb_", "gfti_")}
        assert args["gftb_"] == args["gfti_"], suffix
    assert _series_call.BIGFLOAT_OPS == OPS
    assert bigfloat_series._CALL == _series_call.Call("bigfloat_series", 1, 1, 2048, True, "bigfloat")
    assert _series_call.Call("series", 1, 0, 4096, False).elem is None  # the default: every module from before


def test_module_is_re_exported_and_shares_the_runner():
    import genfer_amd
    from genfer_amd import _series_call, bigfloat_series, interval_series, series

    assert genfer_amd.bigfloat_series is bigfloat_series
    for f in OPS + ("encode", "decode"):
        assert callable(getattr(bigfloat_series, f)) and getattr(bigfloat_series, f).__doc__
    assert bigfloat_series._run is series._run is _series_call.run
    assert bigfloat_series.last_form is series.last_form and bigfloat_series.set_form is series.set_form and bigfloat_series.FORMS is series.FORMS
    assert bigfloat_series.MAX_N == interval_series.MAX_N == 2048
    for f in ("derivative", "shift_down", "observe_chain", "mul_linear", "corr"):  # out of scope: not there
        assert not hasattr(bigfloat_series, f)


# ---- encode / decode ---------------------------------------------------------------------------------------------------------------


def test_encode_decode_match_the_numpy_statements_bit_for_bit():
    torch = pytest.importorskip("torch")
    from genfer_amd import bigfloat
    from genfer_amd import bigfloat_series as bfs

    tiny = np.array([5e-324, -5e-324, 2.2250738585072014e-308, -1.1125369292536007e-308, 3e-310])  # subnormals and the smallest normal
    vals = np.concatenate([[0.0, -0.0, 1.0, -1.0, 1.5, -1.9999999999999998, 2.0, 0.5, INF, -INF, NAN, 1.7976931348623157e308, 3.0e-300, -7.25],
                           tiny, (splitmix64_uniform(11, 64) - 0.5) * 2.0 ** np.arange(-32, 32)])
    for off in (0, 5, -3000, 4000):
        f, e = bigfloat.encode(vals, off)
        got = bfs.encode(torch.from_numpy(vals), off)
        assert tuple(got.shape) == (2,) + vals.shape and got.dtype == torch.float64
        assert same_bits(got.numpy(), np.stack([f, e])), off
        assert np.array_equal(np.signbit(got[0].numpy()), np.signbit(f))  # zeros of either sign give +0
    m = bfs.encode(torch.from_numpy(vals[:81].reshape(3, 3, 9)))  # [2, *t.shape]
    assert tuple(m.shape) == (2, 3, 3, 9)
    # decode: the powi window -1023 / -1024 / 1023 / 1024 and beyond, zeros, infinities (inf * 0 is NaN), NaN
    fs = np.array([1.0, 1.5, -1.75, 1.9999999999999998, 0.0, -0.0, INF, -INF, NAN])
    es = np.array([-3000.0, -1075.0, -1074.0, -1025.0, -1024.0, -1023.0, -1022.0, -1.0, 0.0, 1.0, 1022.0, 1023.0, 1024.0, 1025.0, 3000.0])
    F, E = np.meshgrid(fs, es, indexing="ij")
    want = bigfloat.decode(F, E)
    got = bfs.decode(torch.from_numpy(np.stack([F, E]))).numpy()
    assert same_bits(got, want)
    assert got[0, 4] == 0.0 and got[0, 5] == 2.0**-1023 and got[0, 11] == 2.0**1023 and got[0, 12] == INF and np.isnan(got[6, 4])
    # round trip on the finite values of the normal range (subnormals lie below the powi window: to_f64 gives 0), and with an offset
    fin = vals[np.isfinite(vals) & ((vals == 0.0) | (np.abs(vals) >= 2.0**-1022))]
    assert same_bits(bfs.decode(bfs.encode(torch.from_numpy(fin))).numpy(), fin + 0.0)
    assert bfs.decode(bfs.encode(torch.from_numpy(tiny[[0, 1, 3, 4]]))).tolist() == [0.0, -0.0, -(2.0**-1023), 0.0]  # (-1023 is inside the window)
    x = torch.from_numpy(np.array([1.5, -3.0, 0.0]))
    up = bfs.encode(x, 2000)
    assert up[1].tolist() == [2000.0, 2001.0, 0.0] and bfs.decode(up).tolist() == [INF, -INF, 0.0]
    with pytest.raises(TypeError, match="float64"):
        bfs.encode(x.float())
    with pytest.raises(TypeError, match=r"\[2, \.\.\.\]"):
        bfs.decode(x)


# ---- the Python side's refusals ----------------------------------------------------------------------------------------------------


def _device_like(torch, shape):
    """a tensor without storage (meta) that reports a GPU placement, as tests/make_series_refusals.py builds them: it passes the
    placement check, so the checks in front of it are reached without a device"""

    class Fake(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)

    return torch.zeros(shape, dtype=torch.float64, device="meta").as_subclass(Fake)


def _calls(bfs, x, y=None, n=None, out=None, seed=None):
    y = x if y is None else y
    return [("mul", lambda: bfs.mul(x, y, n=n, out=out)), ("div", lambda: bfs.div(x, y, n=n, out=out)),
            ("compose", lambda: bfs.compose(x, y, n=n, out=out)), ("exp", lambda: bfs.exp(x, n=n, seed=seed, out=out)),
            ("log", lambda: bfs.log(x, n=n, seed=seed, out=out)), ("pow", lambda: bfs.pow(x, 3, n=n, out=out))]


def test_python_side_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    from genfer_amd import bigfloat_series as bfs
    from genfer_amd.taylor import TaylorError

    cpu = torch.zeros((2, 3, 8), dtype=torch.float64)
    d = _device_like(torch, (2, 3, 8))
    for name, f in _calls(bfs, cpu):
        with pytest.raises(TaylorError, match=f"bigfloat_series.{name}: .*on cpu"):
            f()
    for name, f in _calls(bfs, cpu.float()):
        with pytest.raises(TaylorError, match="float32"):  # dtype
            f()
    with pytest.raises(TypeError, match="torch.Tensor"):
        bfs.mul([1.0, 2.0], cpu)
    # the first axis holds the two planes
    for bad in ((3, 3, 8), (1, 3, 8), (3, 8)):
        for name, f in _calls(bfs, _device_like(torch, bad), d):
            with pytest.raises(TaylorError, match=r"a BigFloat tensor is stacked \[2, \.\.\.\] = \(factor, exponent\)"):
                f()
        with pytest.raises(TaylorError, match=r"y: .*stacked \[2, \.\.\.\]"):
            bfs.mul(d, _device_like(torch, bad))
    with pytest.raises(TaylorError, match=r"seed: .*stacked \[2, \.\.\.\]"):
        bfs.exp(d, seed=_device_like(torch, (3,)))
    with pytest.raises(TaylorError, match="no series axis"):
        bfs.mul(_device_like(torch, (2,)), d)
    # unit stride on the series axis
    for name, f in _calls(bfs, _device_like(torch, (2, 3, 16))[..., ::2], d):
        with pytest.raises(TaylorError, match="unit stride"):
            f()
    # the orders: n > 2048, n == 0, an operand longer than n
    for name, f in _calls(bfs, d, n=2049):
        with pytest.raises(TaylorError, match="2048"):
            f()
    for name, f in _calls(bfs, d, n=0):
        with pytest.raises(TaylorError, match="n == 0"):
            f()
    for name, f in _calls(bfs, d, n=6):
        with pytest.raises(TaylorError, match="nx > n"):
            f()
    with pytest.raises(TaylorError, match="nx > n"):
        bfs.div(_device_like(torch, (2, 3, 5)), d, n=6)  # the second operand too
    # plane stride 0: a factor plane cannot be its own exponent plane -- on either operand and on the seeds
    flat = _device_like(torch, (3, 8)).expand(2, 3, 8)
    assert flat.stride(0) == 0
    for name, f in _calls(bfs, flat, d):
        with pytest.raises(TaylorError, match=f"bigfloat_series.{name}: (x|f): .*plane stride 0 .*factor plane cannot be its own exponent plane"):
            f()
    for f in (bfs.mul, bfs.div, bfs.compose):
        with pytest.raises(TaylorError, match="(y|g): .*plane stride 0"):
            f(d, flat)
    for f in (bfs.exp, bfs.log):
        with pytest.raises(TaylorError, match="seed: .*plane stride 0"):
            f(d, seed=_device_like(torch, (3,)).expand(2, 3))
    # out: its shape, its batch
    for name, f in _calls(bfs, d, out=_device_like(torch, (2, 3, 9)), n=8):
        with pytest.raises(TaylorError, match="out has 9 coefficients per series, the result has n = 8"):
            f()
    for name, f in _calls(bfs, d, out=_device_like(torch, (2, 4, 8))):
        with pytest.raises((TaylorError, RuntimeError)):
            f()
    with pytest.raises(TaylorError, match=r"out: .*stacked \[2, \.\.\.\]"):
        bfs.mul(d, d, out=_device_like(torch, (3, 3, 8)))
    # a raw layer: a tracked operand is refused while grad mode is on (series3's wording), and runs into the next check without it
    t = _device_like(torch, (2, 3, 8)).requires_grad_(True)
    for name, f in _calls(bfs, t, d):
        with pytest.raises(TaylorError, match="an operand requires grad, and this version of bigfloat_series has no autograd; pass (x|f).detach\\(\\) or "
                                              "call under torch.no_grad\\(\\) \\(nothing is detached silently\\)"):
            f()
    with pytest.raises(TaylorError, match="requires grad"):
        bfs.mul(d, t)
    # pow's exponent is judged before anything else
    with pytest.raises(TaylorError, match="negative .*bigfloat_series.div"):
        bfs.pow(cpu, -1)
    for bad in (2.5, "3", None, True):
        with pytest.raises(TypeError, match="non-negative integer"):
            bfs.pow(cpu, bad)
    with pytest.raises(TaylorError, match="32 bits"):
        bfs.pow(cpu, 2**32)


def test_interval_modules_keep_their_words():
    """the element kind changes no message of the interval modules: a point interval (plane stride 0) is still a value there"""
    torch = pytest.importorskip("torch")
    from genfer_amd import interval_series as ivs
    from genfer_amd.taylor import TaylorError

    with pytest.raises(TaylorError, match=r"an interval tensor is stacked \[2, \.\.\.\] = \(lo, hi\) along its first axis"):
        ivs.mul(_device_like(torch, (3, 3, 8)), _device_like(torch, (2, 3, 8)))
    with pytest.raises(TaylorError, match="on cpu"):  # the stride check does not fire: the placement is the first thing wrong
        ivs.mul(torch.zeros((3, 8), dtype=torch.float64).expand(2, 3, 8), torch.zeros((2, 3, 8), dtype=torch.float64))


# ---- the C layer's refusals --------------------------------------------------------------------------------------------------------


def test_series_args_on_bigfloat_calls(tmp_path):
    """tests/series_bigfloat_args_main.cpp: a plain host program over gft_series_args.hpp -- the admitted calls, rank and operation,
    plane stride 0 on every tensor, the interval path's judgement unchanged, and an interval and an f64 call under the default element
    kind; under AddressSanitizer and UndefinedBehaviorSanitizer where the compiler has them and the program runs with them.  The
    program is run directly in the inherited environment."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "argsb")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "series_bigfloat_args_main.cpp")]
    for extra in (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []):
        if subprocess.run(base + extra, capture_output=True).returncode != 0:
            continue
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        if extra and out.returncode != 0 and "FAILED" not in out.stdout:
            continue  # (the sanitizers' runtime does not start here: the plain build decides)
        assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
        m = re.search(r"^ok (\d+) checks$", out.stdout.strip().splitlines()[-1])
        assert m and int(m.group(1)) >= 80, out.stdout
        return
    pytest.fail("tests/series_bigfloat_args_main.cpp does not build")


# ---- the gfx950 code ---------------------------------------------------------------------------------------------------------------


def test_bigfloat_series_isa(tmp_path):
    """The gfx950 code of the BigFloat instantiations (tests/series_bigfloat_isa_check.hip): no scratch and no spill in any kernel
    (.private_segment_fixed_size 0, as DESIGN 3.29 records), and no contraction -- no FMA of any spelling in the mul and compose
    kernels, in the div kernel the five of each IEEE f64 division sequence (v_div_fmas_f64), in the exp / log kernels those and exactly
    the FMAs of EBig::exp / log (the device library's exp2 / log2), counted on the file's two probe kernels.  It looks for nothing else."""
    import glob

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", "series_bigfloat_isa_check.hip")],
                          cwd=tmp_path)
    isa = open(glob.glob(str(tmp_path / "*amdgcn-amd-amdhsa*gfx950*.s"))[0]).read()
    assert isa.count(".private_segment_fixed_size: 0") == 9 and isa.count(".private_segment_fixed_size:") == 9
    assert isa.count(".vgpr_spill_count: 0") == 9 and isa.count(".sgpr_spill_count: 0") == 9
    kernels = {}
    name = None
    for line in isa.splitlines():
        m = re.match(r"^(_ZN3gft\w+):", line)
        if m:
            name = m.group(1)
            kernels[name] = []
        elif line.startswith("\t.end_amdhsa_kernel") or line.startswith("\t.section"):
            name = None
        elif name and line.startswith("\t") and not line.lstrip().startswith("."):
            kernels[name].append(line.split()[0])

    def one(*parts):
        got = [c for k, c in kernels.items() if all(p in k for p in parts)]
        assert len(got) == 1 and len(got[0]) > 50, parts
        return got[0]

    fmas = lambda code: sum(("fma" in c and c != "v_div_fmas_f64") or c.startswith("v_fmac") or c.startswith("v_mad_f64") for c in code)  # noqa: E731
    mul_a, div_a, compose_a = one("k_series_mul_a", "EBig"), one("k_series_div_a", "EBig"), one("k_series_compose_a", "EBig")
    exp_a, log_a = one("k_series_explog_a", "EBigELb0"), one("k_series_explog_a", "EBigELb1")
    mul_b, compose_b = one("k_series_mul_b", "EBig"), one("k_series_compose_b", "EBigELb1")
    for code in (mul_a, compose_a, mul_b, compose_b):
        assert fmas(code) == 0, "a contracted multiply-add"
    assert div_a.count("v_div_fmas_f64") >= 1 and fmas(div_a) == 5 * div_a.count("v_div_fmas_f64")
    for log, code in ((0, exp_a), (1, log_a)):
        probe = one("k_seed_probe", f"Lb{log}")
        assert probe.count("v_div_fmas_f64") == 0 and code.count("v_div_fmas_f64") >= 1
        assert fmas(code) == 5 * code.count("v_div_fmas_f64") + fmas(probe), (log, fmas(code), fmas(probe))


# ---- the expected values -----------------------------------------------------------------------------------------------------------


def test_data_is_what_it_says():
    for kind in KINDS:
        X = data(kind, 40, 33, 5)
        f, e = X
        assert np.all(e == np.floor(e)) and np.all(np.abs(e) <= 3000)
        ok = ((np.abs(f) >= 1.0) & (np.abs(f) < 2.0)) | ((f == 0.0) & (e == 0.0)) | ~np.isfinite(f)
        assert ok.all()
        assert np.all(f[:, 0] >= 1.0)
    w = data("wide", 40, 33, 5)
    assert w[1].min() < -2500 and w[1].max() > 2500 and np.abs(np.diff(w[1], axis=1)).max() > 1023 and (w[0] < 0).any()
    t = data("tiny", 40, 33, 5)
    assert (t[1] <= -1024).any() and ((t[0] == 0) & ~np.signbit(t[0])).any() and ((t[0] == 0) & np.signbit(t[0])).any()
    s = data("special", 40, 33, 5)
    assert np.isnan(s[0]).any() and (s[0] == INF).any() and (s[0] == -INF).any() and (s[1][~np.isfinite(s[0])] != 0).any()
    h = data("wide", 40, 8, 5, EXP_HEAD)
    assert h[1][:, 0].min() >= EXP_HEAD[0] and h[1][:, 0].max() <= EXP_HEAD[1]


def test_raw_product_equals_the_oracle_operator(orcb, OTPB):
    """on rows with both lengths >= 3 the oracle's `*` takes none of its shortcuts (they look at the stored shapes: zero, one, constant,
    linear; mt:1014-1072) and runs mul_rec: orcb_series_mul_raw is that product -- the sums of mul_1d added onto a zeroed result"""
    for n, nx, ny in [(3, 3, 3), (7, 4, 7), (16, 16, 16), (33, 20, 33), (64, 64, 40), (129, 129, 129)]:
        for kind in KINDS:
            X, Y = data(kind, 3, nx, 100 * n + nx), data(kind, 3, ny, 200 * n + ny + 1)
            want = np.stack([pad((OTPB.new(X[:, b], (n,)) * OTPB.new(Y[:, b], (n,))).array(), n) for b in range(3)], axis=1)
            assert same_bits(want_mul(orcb, X, Y, n), want), (n, nx, ny, kind)


def test_raw_product_is_the_written_definition_and_its_zero_matters(orcb):
    """z[k] = 0 + (0 + x[lo] * y[k - lo] + ...) in scalar BigFloat operations; and the outer 0 + is not idle: a sum at exponent -1023
    loses its last bit to it, one below is dropped -- a kernel that skips it differs"""
    s = lambda code, a, b=None: scalar_op(orcb, code, a, b)  # noqa: E731
    for kind in KINDS:
        for n, nx, ny in [(9, 9, 9), (12, 5, 8), (6, 1, 6)]:
            X, Y = data(kind, 4, nx, 7 * n + nx), data(kind, 4, ny, 9 * n + ny)
            for b in range(4):
                z = []
                for k in range(n):
                    acc = ZERO
                    for j in range(max(0, k + 1 - ny), min(k + 1, nx)):
                        acc = s(0, acc, s(2, X[:, b, j], Y[:, b, k - j]))
                    z.append(s(0, ZERO, acc))
                assert same_bits(mul_raw(orcb, X[:, b], Y[:, b], n), np.array(z).T), (kind, n, nx, ny, b)
    # the crafted operands: the sum of coefficient 1 is a residual at exponent -1042 (mul) / -1039 (compose's second step), the result 0
    x, y, n = crafted()["mul"]
    acc = s(0, s(0, ZERO, s(2, x[:, 0], y[:, 1])), s(2, x[:, 1], y[:, 0]))
    assert acc[0] != 0.0 and acc[1] == -1042.0 and s(0, ZERO, acc).tolist() == [0.0, 0.0]
    assert mul_raw(orcb, x, y, n).tolist() == [[1.125, 0.0], [-1021.0, 0.0]]
    f, g, n = crafted()["compose"]
    assert chain_compose(orcb, f, g, n).tolist() == [[1.0, 0.0, 1.125], [0.0, 0.0, -1019.0]]
    r0 = s(0, s(0, ZERO, s(2, f[:, 2], g[:, 0])), f[:, 1])  # (f2 * g0 + f1 after the first step)
    acc = s(0, s(0, ZERO, s(2, r0, g[:, 1])), s(2, s(2, f[:, 2], g[:, 1]), g[:, 0]))
    assert acc.tolist() == [-1.5, -1039.0]
    odd = np.array([[1.0000000000000002], [-1023.0]])  # an odd last bit at exponent -1023
    one = np.array([[1.0], [0.0]])
    assert mul_raw(orcb, odd, one, 1).ravel().tolist() == [1.0, -1023.0]
    assert mul_raw(orcb, np.array([[1.5], [-1024.0]]), one, 1).ravel().tolist() == [0.0, 0.0]
    assert chain_compose(orcb, np.array([[1.5], [-1024.0]]), np.array([[1.0, 1.0], [0.0, 0.0]]), 3).tolist() == [[0.0] * 3, [0.0] * 3]  # one slice: 0 + f


def test_handle_operators_are_the_written_definitions(orcb, OTPB):
    """div / exp / log through the oracle's handle operators equal the loops written out in scalar operations (no extra addition of
    zero in these: their sums are stored as formed)"""
    for kind in KINDS:
        for op in ("div", "exp", "log"):
            for n, nx, ny in [(2, 2, 2), (7, 7, 7), (9, 4, 8), (12, 12, 2)]:
                X, Y = operands(op, kind, n, 3, nx, ny)
                if op != "div":
                    Y = None
                want = want_handle(orcb, OTPB, op, X, Y, n)
                for b in range(3):
                    got = define(orcb, op, X[:, b], None if Y is None else Y[:, b], n)
                    assert same_bits(got, want[:, b]), (kind, op, n, nx, ny, b)


def test_chains_equal_the_oracle_subst_var_and_pow(orcb, OTPB):
    """The oracle's subst_var and pow are the chains wherever BigFloat's 0 + b returns b: their first product is a shortcut (a constant
    times g is c * g[k], 1 * base is base) where the batched layer runs the general product 0 + (0 + c * g[k]), as for f64 and
    intervals -- the same value on rows whose exponents stay near 0 (for ng >= 3, where subst_var takes its Horner path)."""
    for n, nf, ng in [(3, 3, 3), (7, 5, 4), (16, 16, 16), (33, 9, 33), (40, 40, 3), (64, 2, 64), (64, 1, 5)]:
        F, G = data("near", 3, nf, 300 * n + nf), data("near", 3, ng, 500 * n + ng + 7)
        want = np.stack([pad(OTPB.new(F[:, b], (n,)).subst_var(0, OTPB.new(G[:, b], (n,))).array(), n) for b in range(3)], axis=1)
        assert same_bits(want_compose(orcb, F, G, n), want), ("compose", n, nf, ng)
    for n, nx in [(16, 16), (40, 9), (64, 64)]:
        X = data("near", 3, nx, 700 * n + nx)
        for e in (1, 2, 3, 5, 8, 11):
            want = np.stack([pad(OTPB.new(X[:, b], (n,)).pow(e).array(), n) for b in range(3)], axis=1)
            assert same_bits(want_pow(orcb, X, e, n), want), ("pow", n, nx, e)
    # and where 0 + b does not return b the chain, not the shortcut, is the definition: the general product of every step
    F, G = np.array([[1.0, 1.5], [0.0, -1000.0]]), np.array([[1.0, 1.25, 1.0], [0.0, -30.0, 0.0]])
    got = chain_compose(orcb, F, G, 3)  # step 1: 0 + (0 + {1.5, -1000} * g[k]); g[1]'s product lies at -1030 and is dropped
    assert got.tolist() == [[1.0, 0.0, 1.5], [0.0, 0.0, -1000.0]]
    assert OTPB.new(F, (3,)).subst_var(0, OTPB.new(G, (3,))).array()[:, 1].tolist() == [1.875, -1030.0]


def test_compose_chain_is_the_written_definition(orcb):
    """the compose chain against the loops of the definition written out in scalar BigFloat operations, on every kind of row, ng <= 2
    too (where the oracle's operators would shortcut)"""
    s = lambda code, a, b=None: scalar_op(orcb, code, a, b)  # noqa: E731
    for kind in KINDS:
        for n, nf, ng in [(6, 3, 2), (4, 1, 3), (5, 4, 1), (7, 4, 3), (9, 5, 9)]:
            F, G = data(kind, 2, nf, 41 * n + nf), data(kind, 2, ng, 43 * n + ng)
            for b in range(2):
                f, g = F[:, b], G[:, b]
                res = [s(0, ZERO, f[:, nf - 1])]
                for i in range(nf - 2, -1, -1):
                    new = []
                    for k in range(min(len(res) + ng - 1, n)):
                        acc = ZERO
                        for j in range(max(0, k + 1 - ng), min(k + 1, len(res))):
                            acc = s(0, acc, s(2, res[j], g[:, k - j]))
                        new.append(s(0, ZERO, acc))
                    new[0] = s(0, new[0], f[:, i])
                    res = new
                assert same_bits(chain_compose(orcb, f, g, n), pad(np.array(res).T, n)), (kind, n, nf, ng, b)


def test_finite_cases_stay_finite(orcb, OTPB):
    """every expected value of the GPU test's finite cases: no NaN and no inf anywhere -- so the GPU comparison is bit equality on 100 % of
    the coefficients with nothing masked; and the seeds the GPU test hands over are finite too"""
    with np.errstate(all="ignore"):
        for op in OPS:
            for kind in FINITE:
                count = 0
                for n, B, nx, ny, e, _forms in bit_exact_cases(op):
                    X, Y, want = expected(orcb, OTPB, op, kind, n, B, nx, ny, e)
                    assert want.shape == (2, B, n)
                    assert np.isfinite(want).all(), (op, kind, n, B, nx, ny, e)
                    f, x = want
                    ok = ((np.abs(f) >= 1.0) & (np.abs(f) < 2.0)) | ((f == 0.0) & (x == 0.0))
                    assert ok.all() and np.all(x == np.floor(x)) and np.abs(x).max() < 2.0**31, (op, kind, n)
                    if op in ("exp", "log"):
                        assert np.isfinite(host_seeds(orcb, op, X)).all()
                    count += 1
                assert count >= len(ORDERS)
    # the special rows do carry what they are for
    X, Y, want = expected(orcb, OTPB, "mul", "special", 9, 6, 9, 9)
    assert np.isnan(want[0]).any() and np.isinf(want[0]).any() and np.isfinite(want[1]).all()
