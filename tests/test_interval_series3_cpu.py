"""Batched trivariate interval series (genfer_amd.interval_series3, gfti_series3_*) without a GPU: the exported and declared surface,
the refusals the Python side makes before it touches the library, the host argument layer on rank-3 interval calls
(tests/series3_interval_args_main.cpp, also under the sanitizers), and the expected values themselves -- the raw interval product of
tests/series3_interval_oracle.cpp against the oracle's operator, the model of tests/_series3_interval_model.py against that product
and against the oracle's handle operators, the compose / pow chains against the oracle's subst_var / pow, and the sentinels of the two
shape rules (tests/test_interval_series3_gpu.py imports the data and the expected values from this file)."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _series3_compose_cases as cc
import _series3_interval_model as model
from _series3_model import result_shape
from _series3_oracle import dense, signed
from conftest import ROOT, splitmix64_uniform
from test_interval_series2_cpu import assert_bits, bits_equal  # noqa: F401  (re-exported)
from test_interval_series_cpu import _device_like, data, scalar_add, scalar_fn

SYMBOLS = tuple("gfti_series3_" + op for op in ("mul", "div", "exp", "log", "compose", "pow"))
OPS = ("mul", "div", "exp", "log")
KINDS = ("dense", "signed")

# ---- the expected values shared with the GPU tests ----------------------------------------------------------------------------

_SHIM = {}


def shim_lib(tmp_root):
    """tests/series3_interval_oracle.cpp: the oracle's mul_rec<Interval> at rank 3 on plane-major buffers (built once per session)"""
    if "lib" not in _SHIM:
        so = os.path.join(str(tmp_root), "liborcis3.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so,
                               os.path.join(ROOT, "tests", "series3_interval_oracle.cpp")])
        L = C.CDLL(so)
        L.orci_series3_mul_raw.restype = C.c_int
        L.orci_series3_mul_raw.argtypes = [C.c_void_p] + [C.c_size_t] * 3 + [C.c_void_p] + [C.c_size_t] * 3 + [C.c_void_p] + [C.c_size_t] * 3
        _SHIM["lib"] = L
    return _SHIM["lib"]


@pytest.fixture(scope="session")
def shim3(tmp_path_factory):
    return shim_lib(tmp_path_factory.mktemp("orcis3"))


def data3(kind, B, shape, seed):
    """[2, B, n0, n1, n2] interval items.  "dense" / "signed": the f64 data of tests/_series3_oracle.py as the lower bounds, every
    upper bound a positive width above (about 2^-20 relative to 1), and every third item a point interval.  "special": the rows of
    test_interval_series_cpu.data over the row-major item (an exact [0,0] and one of [1,1], [-1,-1], an infinity, a NaN, [0,0] seeded
    past coefficient [0, 0, 0], which stays in [0.5, 1.5))"""
    shape = tuple(shape)
    if kind == "special":
        return data(kind, B, int(np.prod(shape)), seed).reshape((2, B) + shape)
    lo = (signed if kind == "signed" else dense)((B,) + shape, seed)
    w = (0.25 + splitmix64_uniform(seed + 977, lo.size).reshape(lo.shape)) * 2.0**-20
    w[::3] = 0.0
    return np.stack([lo, lo + w])


def pad3i(a, n):
    """[2, s0, s1, s2] (or fewer axes, as the oracle stores a constant) -> [2, n0, n1, n2], +0 beyond"""
    a = np.asarray(a, dtype=np.float64)
    a = a.reshape(a.shape + (1,) * (4 - a.ndim))
    out = np.zeros((2,) + tuple(n))
    out[:, :a.shape[1], :a.shape[2], :a.shape[3]] = a
    return out


def mul_raw3(shim, x, y, n):
    """the shim on one item at the stored result shape S = min(n, nx + ny - 1) (the oracle squeezes its unit axes itself: mul_rec's
    one-long-axis case), extended with +0 to n: x [2, nx0, nx1, nx2], y [2, ny0, ny1, ny2] -> [2, n0, n1, n2]"""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    s = result_shape("mul", tuple(n), x.shape[1:], y.shape[1:])
    out = np.zeros((2,) + s)
    assert shim.orci_series3_mul_raw(C.c_void_p(x.ctypes.data), *x.shape[1:], C.c_void_p(y.ctypes.data), *y.shape[1:], C.c_void_p(out.ctypes.data), *s) == 0
    return pad3i(out, n)


def want_mul(shim, X, Y, n):
    return np.stack([mul_raw3(shim, X[:, b], Y[:, b], n) for b in range(X.shape[1])], axis=1)


def want_handle(OTPI, op, X, Y, n):
    """div / exp / log through the oracle's handle operators per item"""
    out = []
    for b in range(X.shape[1]):
        p = OTPI.new(X[:, b], n)
        r = p / OTPI.new(Y[:, b], n) if op == "div" else (p.exp() if op == "exp" else p.log())
        out.append(pad3i(r.array(), n))
    return np.stack(out, axis=1)


def is_normative(op, X, Y):
    """The classes on which the loops, not the oracle's operators, are the definition -- by shape rule: a divisor of ONE stored
    coefficient (the operator's constant shortcut, as at f64), and exp of an operand that is a single row or column (at most one
    non-unit axis) holding an infinity or a NaN (the oracle then leaves the rest of the result +0 where the definition multiplies
    by the [0,0] there)."""
    if op == "div":
        return int(np.prod(Y.shape[-3:])) > 1
    if op == "exp" and sum(v > 1 for v in X.shape[-3:]) <= 1:
        return bool(np.isfinite(X).all())
    return True


def host_seeds(oracle_lib, op, X):
    """[2, B]: the interval exp / ln of coefficient [0, 0, 0] per item"""
    return np.stack([scalar_fn(oracle_lib, op, X[:, b, 0, 0, 0]) for b in range(X.shape[1])], axis=1)


def want_model(oracle_lib, op, X, Y, n, seeds=None, **kw):
    o = model.Ops(oracle_lib)
    out = []
    for b in range(X.shape[1]):
        if op in ("mul", "div"):
            out.append(getattr(model, op)(o, X[:, b], Y[:, b], n, **kw))
        else:
            sd = seeds[:, b] if seeds is not None else scalar_fn(oracle_lib, op, X[:, b, 0, 0, 0])
            out.append(getattr(model, op)(o, X[:, b], n, sd, **kw))
    return np.stack(out, axis=1)


def chain_compose(mul, oracle_lib, f, g, var, n):
    """3.23's chain over intervals: Horner over the slices of f along axis var, every product `mul(a, b, L)` at the compact shape of the
    step, the slice add the oracle's scalar add"""
    f, g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
    add = lambda a, b: scalar_add(oracle_lib, a, b)  # noqa: E731
    cut = lambda i: (slice(None),) + tuple(slice(i, i + 1) if a == var else slice(None) for a in range(3))  # noqa: E731

    def added(res, s):
        for idx in itertools.product(*[range(v) for v in s.shape[1:]]):
            at = (slice(None),) + idx
            res[at] = add(res[at], s[at])
        return res

    last = f[cut(f.shape[1 + var] - 1)]
    res = added(np.zeros(last.shape), last)
    for i in range(f.shape[1 + var] - 2, -1, -1):
        res = added(np.array(mul(res, g, cc.compact(res.shape[1:], g.shape[1:], n))), f[cut(i)])
    return pad3i(res, n)


def chain_pow(mul, x, e, n):
    """square-and-multiply without the last squaring, compact shapes, from [[[[1,1]]]]"""
    res, base = np.ones((2, 1, 1, 1)), np.array(x, dtype=np.float64)
    while e > 0:
        if e & 1:
            res = mul(res, base, cc.compact(res.shape[1:], base.shape[1:], n))
        e >>= 1
        if e > 0:
            base = mul(base, base, cc.compact(base.shape[1:], base.shape[1:], n))
    return pad3i(res, n)


def want_compose(shim, oracle_lib, F, G, var, n):
    mul = lambda a, b, L: mul_raw3(shim, a, b, L)  # noqa: E731
    return np.stack([chain_compose(mul, oracle_lib, F[:, b], G[:, b], var, n) for b in range(F.shape[1])], axis=1)


def want_pow(shim, X, e, n):
    mul = lambda a, b, L: mul_raw3(shim, a, b, L)  # noqa: E731
    return np.stack([chain_pow(mul, X[:, b], e, n) for b in range(X.shape[1])], axis=1)


# ---- the surface -----------------------------------------------------------------------------------------------------------------


def test_symbols_are_declared_and_exported():
    import genfer_amd

    if not os.path.exists(genfer_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    L = genfer_amd.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert hasattr(L, s), s
        assert f"pub fn {s}(" in doc, s
    assert re.search(r"gfti_series3_pow\([^)]*uint32_t\s+e\b", header)
    assert re.search(r"gfti_series3_compose\([^)]*int\s+var\b", header)
    from genfer_amd import _series_call

    D = _series_call._lib()
    for s in SYMBOLS:  # declared from the one table, the f64 twin's argument list
        assert getattr(D, s).argtypes == getattr(D, s.replace("gfti_", "gft_")).argtypes and getattr(D, s).restype is C.c_int


def test_module_is_re_exported_and_shares_the_runner():
    import genfer_amd
    from genfer_amd import _series_call, interval_series3, series3

    assert genfer_amd.interval_series3 is interval_series3
    for f in ("mul", "div", "exp", "log", "compose", "pow"):
        assert callable(getattr(interval_series3, f)) and getattr(interval_series3, f).__doc__
    assert interval_series3._run is series3._run is _series_call.run
    assert interval_series3.MAX_ELEMS == 2048 and series3.MAX_ELEMS == 4096
    assert interval_series3._CALL == _series_call.Call("interval_series3", 3, 1, 2048, True)


def test_python_side_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    from genfer_amd import interval_series3 as ivs3
    from genfer_amd import series3
    from genfer_amd.taylor import TaylorError

    d = _device_like(torch, (2, 3, 2, 4, 8))
    # planes missing: the plane axis and three series axes
    for bad in ((2, 4, 8), (2, 8), (2,)):
        with pytest.raises(TaylorError, match="trivariate interval series needs at least 4"):
            ivs3.mul(_device_like(torch, bad), d)
        with pytest.raises(TaylorError, match="y: .*needs at least 4"):
            ivs3.mul(d, _device_like(torch, bad))
    with pytest.raises(TaylorError, match=r"stacked \[2, \.\.\.\]"):
        ivs3.mul(_device_like(torch, (3, 3, 2, 4, 8)), d)
    with pytest.raises(TaylorError, match=r"seed: .*stacked \[2, \.\.\.\]"):
        ivs3.exp(d, seed=_device_like(torch, (3,)))
    for bad in ((2, 3, 0, 4, 8), (2, 3, 2, 0, 8), (2, 3, 2, 4, 0)):
        with pytest.raises(TaylorError, match="a series axis is empty"):
            ivs3.exp(_device_like(torch, bad))
    with pytest.raises(TaylorError, match="unit stride"):
        ivs3.mul(_device_like(torch, (2, 3, 2, 4, 16))[..., ::2], d)
    # the limit is 2048 coefficients, with its text; the f64 family keeps 4096
    big = _device_like(torch, (2, 1, 2, 2, 4))
    for call in (lambda n: ivs3.mul(big, big, n=n), lambda n: ivs3.div(big, big, n=n), lambda n: ivs3.exp(big, n=n), lambda n: ivs3.log(big, n=n),
                 lambda n: ivs3.compose(big, big, 0, n=n), lambda n: ivs3.pow(big, 3, n=n)):
        with pytest.raises(TaylorError, match=r"n0 \* n1 \* n2 = 3 \* 683 \* 1 = 2049 exceeds the limit of 2048 coefficients per item"):
            call((3, 683, 1))
        with pytest.raises(TaylorError, match=r"= 2 \* 2 \* 513 = 2052 exceeds the limit of 2048"):
            call((2, 2, 513))
        for n in [(1, 2, 4), (2, 1, 4), (2, 2, 3)]:  # n shorter than an operand, on each axis
            with pytest.raises(TaylorError, match="nx > n"):
                call(n)
        with pytest.raises(TaylorError, match="n == 0"):
            call((2, 0, 4))
        with pytest.raises(TypeError, match="triple"):
            call((4, 8))
    assert series3._orders("t", (16, 16, 16), (1, 1, 1)) == (16, 16, 16)
    # var, the exponent
    for bad in (3, -1, 1.0, True, None):
        with pytest.raises(TaylorError, match=r"interval_series3.compose: var = .*is 0 \(axis -3\), 1 \(axis -2\) or 2 \(axis -1\)"):
            ivs3.compose(d, d, var=bad)
    with pytest.raises(TaylorError, match="negative"):
        ivs3.pow(d, -1)
    with pytest.raises(TypeError, match="non-negative integer"):
        ivs3.pow(d, 2.5)
    # a tracked operand: refused as in series3
    x = torch.zeros((2, 3, 2, 4, 8), dtype=torch.float64, requires_grad=True)
    with pytest.raises(TaylorError, match="interval_series3 has no autograd"):
        ivs3.mul(x, x.detach())
    with pytest.raises(TaylorError, match="no autograd"):
        ivs3.exp(x)
    with torch.no_grad():  # (grad mode off: the check passes and the placement, judged last, refuses)
        with pytest.raises(TaylorError, match="on cpu"):
            ivs3.exp(x)
    # out of the wrong shape
    with pytest.raises(TaylorError, match=r"out has \(2, 4, 9\) coefficients per item"):
        ivs3.mul(d, d, out=_device_like(torch, (2, 3, 2, 4, 9)))
    with pytest.raises(TaylorError, match="out has batch shape"):
        ivs3.mul(d, d, out=_device_like(torch, (2, 1, 2, 4, 8)))
    with pytest.raises(TaylorError, match=r"out: .*stacked \[2, \.\.\.\]"):
        ivs3.mul(d, d, out=_device_like(torch, (1, 3, 2, 4, 8)))
    with pytest.raises(TaylorError, match="on cpu"):
        ivs3.mul(x.detach(), x.detach())
    with pytest.raises(TaylorError, match="float32"):
        ivs3.mul(x.detach().float(), d)


def test_bench_series3_has_the_interval_mode():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_series3.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "--interval" in out.stdout


# ---- the host argument layer ----------------------------------------------------------------------------------------------------


def test_series_args_on_rank3_interval_calls(tmp_path):
    """tests/series3_interval_args_main.cpp: a plain host program over gft_series_args.hpp -- the limit, the plane stride's place, plane
    overlap of the result, pow's cap on non-contiguous axes, the unchanged text of an operation rank 3 lacks, the device-free plans;
    under AddressSanitizer and UndefinedBehaviorSanitizer where the compiler has them and the program runs with them.  The program is
    run directly in the inherited environment, as tests/test_series3_compose_cpu.py runs its own"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "args3i")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "genfer_amd", "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "series3_interval_args_main.cpp")]
    for extra in (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []):
        if subprocess.run(base + extra, capture_output=True).returncode != 0:
            continue
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        if extra and out.returncode != 0 and "FAILED" not in out.stdout:
            continue  # (the sanitizers' runtime does not start here: the plain build decides)
        assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
        m = re.search(r"^ok (\d+) checks$", out.stdout.strip().splitlines()[-1])
        assert m and int(m.group(1)) >= 30, out.stdout
        return
    pytest.fail("tests/series3_interval_args_main.cpp does not build")


# ---- the expected values -----------------------------------------------------------------------------------------------------------

RESULTS = [(3, 3, 3), (4, 2, 3), (2, 4, 2), (3, 1, 3), (1, 2, 3), (2, 2, 1)]  # tests/test_series3_cpu.py's six result shapes


def stored_lengths(n):
    """every combination of {1, n_a - 1, n_a} per axis"""
    return list(itertools.product(*[sorted({1, max(1, na - 1), na}) for na in n]))


def test_shim_product_equals_the_oracle_operator(OTPI, shim3):
    """on dense items with at least 3 stored coefficients on every axis of both factors the oracle's `*` takes none of its shortcuts
    (zero, one, constant, linear; mt:1014-1072) and runs mul_rec: the shim is that product"""
    checked = 0
    for n, xs, ys in [((3, 3, 3),) * 3, ((3, 4, 5),) * 3, ((5, 3, 4), (3, 3, 4), (4, 3, 3)), ((4, 4, 8), (4, 4, 8), (3, 3, 5)), ((8, 8, 8),) * 3]:
        for kind in KINDS + ("special",):
            X, Y = data3(kind, 3, xs, 100 * n[0] + n[2]), data3(kind, 3, ys, 200 * n[0] + n[2] + 1)
            want = np.stack([pad3i((OTPI.new(X[:, b], n) * OTPI.new(Y[:, b], n)).array(), n) for b in range(3)], axis=1)
            assert_bits(want_mul(shim3, X, Y, n), want, f"mul {n} x{xs} y{ys} {kind}")
            checked += 3
    assert checked == 45


def thinned(n, op):
    """the stored lengths {1, n_a - 1, n_a} per operand axis, thinned: every stored shape of x, against y = n and against one further
    stored shape of y taken in turn (unary ops: every stored shape of x)"""
    shapes = stored_lengths(n)
    if op in ("exp", "log"):
        return [(xs, n) for xs in shapes]
    out = []
    for i, xs in enumerate(shapes):
        out += [(xs, n), (xs, shapes[(5 * i + 3) % len(shapes)])]
    return sorted(set(out + [(n, ys) for ys in shapes]))


def test_model_equals_the_shim_for_mul(oracle_lib, shim3):
    checked = 0
    for n in RESULTS:
        for j, (xs, ys) in enumerate(thinned(n, "mul")):
            kind = KINDS[j % 2]
            X, Y = data3(kind, 2, xs, 7 * n[0] + n[1] + j), data3(kind, 2, ys, 11 * n[0] + n[2] + j)
            assert_bits(want_model(oracle_lib, "mul", X, Y, n), want_mul(shim3, X, Y, n), f"model mul {n} x{xs} y{ys} {kind}")
            checked += 2
    assert checked == CHECKED["mul"], checked


# items compared against the oracle per op: the thinned stored lengths under the six result shapes, two items each
CHECKED = {"mul": 420, "div": 396, "exp": 152, "log": 152}  # (div: less the 24 under a divisor of one stored coefficient)


@pytest.mark.parametrize("op", ["div", "exp", "log"])
def test_model_equals_the_handle_operators(op, OTPI, oracle_lib):
    """the loops written out in scalar interval operations are the oracle's `/`, exp() and log() wherever those are normative: with
    dense and mixed-sign data everywhere but under a divisor of one stored coefficient (counted, not skipped silently)"""
    checked = modelled = 0
    for n in RESULTS:
        for j, (xs, ys) in enumerate(thinned(n, op)):
            kind = KINDS[j % 2]
            X, Y = data3(kind, 2, xs, 7 * n[0] + n[1] + j), data3(kind, 2, ys, 11 * n[0] + n[2] + j)
            if not is_normative(op, X, Y):
                assert op == "div" and ys == (1, 1, 1)
                modelled += 2
                continue
            assert_bits(want_model(oracle_lib, op, X, Y, n), want_handle(OTPI, op, X, Y, n), f"model {op} {n} x{xs} y{ys} {kind}")
            checked += 2
    assert checked == CHECKED[op] and modelled == (CHECKED["mul"] - CHECKED["div"] if op == "div" else 0), (checked, modelled)


def test_chains_equal_the_oracle_subst_var_and_pow(OTPI, shim3, oracle_lib):
    """for g with at least 3 stored coefficients on every axis the oracle's subst_var takes its general Horner path and every product
    the general one; pow likewise"""
    checked = 0
    for n, fs, gs in [((3, 3, 3),) * 3, ((3, 4, 5), (3, 4, 5), (3, 3, 4)), ((4, 4, 8), (2, 4, 8), (4, 4, 8)), ((5, 3, 4), (5, 3, 2), (3, 3, 4))]:
        for var in (0, 1, 2):
            for kind in KINDS + ("special",):
                F, G = data3(kind, 2, fs, 500 * n[0] + n[2] + var), data3(kind, 2, gs, 600 * n[0] + n[2] + 7)
                want = np.stack([pad3i(OTPI.new(F[:, b], n).subst_var(var, OTPI.new(G[:, b], n)).array(), n) for b in range(2)], axis=1)
                assert_bits(want_compose(shim3, oracle_lib, F, G, var, n), want, f"compose var={var} {n} f{fs} g{gs} {kind}")
                checked += 2
    assert checked == 72
    for n, xs in [((3, 3, 3), (3, 3, 3)), ((3, 4, 5), (3, 4, 5)), ((4, 4, 8), (3, 3, 5))]:
        for kind in KINDS + ("special",):
            X = data3(kind, 2, xs, 700 * n[0] + n[2])
            for e in (2, 3, 5, 8):
                want = np.stack([pad3i(OTPI.new(X[:, b], n).pow(e).array(), n) for b in range(2)], axis=1)
                assert_bits(want_pow(shim3, X, e, n), want, f"pow {n} x{xs} e={e} {kind}")
                checked += 2
    assert checked == 72 + 72


def test_the_squeeze_sentinels_hold_for_intervals(OTPI, oracle_lib, shim3):
    """3.22's sentinel of rule 1 and 3.23's of the squeeze, over intervals: a result computed on n instead of S, or by the rank-3 loops in
    the caller's axis order without the squeeze, differs from the oracle in at least one bound"""
    o = model.Ops(oracle_lib)
    # rule 1: exp of x stored as (4, 2, 1) at the result (5, 3, 2); S = (5, 3, 1) carries the oracle's bits
    n = (5, 3, 2)
    X = data3("dense", 1, (4, 2, 1), 5)
    assert result_shape("exp", n, X.shape[2:]) == (5, 3, 1)
    want = want_handle(OTPI, "exp", X, None, n)
    assert_bits(want_model(oracle_lib, "exp", X, None, n), want, "exp on S")
    off = ~bits_equal(want_model(oracle_lib, "exp", X, None, n, on=n), want)
    assert off.any() and not off[..., 1].any(), int(off.sum())
    # the squeeze: mul's product in caller axis order on a shape with a unit axis
    Y = data3("dense", 1, (3, 3, 1), 6)
    Xs = data3("dense", 1, (4, 3, 1), 7)
    L = (5, 4, 1)
    want = want_mul(shim3, Xs, Y, L)
    assert_bits(want_model(oracle_lib, "mul", Xs, Y, L), want, "mul squeezed")
    off2 = ~bits_equal(want_model(oracle_lib, "mul", Xs, Y, L, squeeze=False), want)
    assert off2.any(), "the unsqueezed product associates differently"
    # 3.23's compose sentinels: the chain over the unsqueezed product differs from the chain over the shim's
    counts = []
    for fs, gs, n, var in cc.SENTINELS:
        F, G = data3("dense", 1, fs, 31 + var), data3("dense", 1, gs, 37 + var)
        want = want_compose(shim3, oracle_lib, F, G, var, n)
        unsq = chain_compose(lambda a, b, L: model.mul(o, a, b, L, squeeze=False), oracle_lib, F[:, 0], G[:, 0], var, n)
        sq = chain_compose(lambda a, b, L: model.mul(o, a, b, L), oracle_lib, F[:, 0], G[:, 0], var, n)
        assert_bits(sq, want[:, 0], f"compose chain over the model {fs} {gs}")
        d = ~bits_equal(unsq, want[:, 0])
        assert d.any(), (fs, gs, n, var)
        counts.append(int(d.sum()))
    print("sentinel bounds that differ: on n", int(off.sum()), "unsqueezed mul", int(off2.sum()), "unsqueezed compose", counts)
