"""Batched bivariate interval series (genfer_amd.interval_series2, gfti_series2_*) without a GPU: the exported and declared surface,
the refusals the Python side makes before it touches the library, the measurement tool's command line, the gfx950 code of the
Interval<F64> instantiations of the rank-2 kernels, and the expected values themselves -- the raw interval product of
tests/series2_interval_oracle.cpp against the oracle's operator, the model of tests/_series2_interval_model.py against the oracle's
handle operators, and the compose / pow chains against the oracle's subst_var / pow (tests/test_interval_series2_gpu.py imports
the data and the expected values from this file)."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _series2_interval_model as model
from _series2_oracle import compact_shapes
from conftest import ROOT
from test_interval_series_cpu import _device_like, data, scalar_add, scalar_fn

SYMBOLS = tuple("gfti_series2_" + op for op in ("mul", "div", "exp", "log", "compose", "pow"))
KINDS = ("pos", "mixed", "special")

# ---- the expected values shared with the GPU tests ----------------------------------------------------------------------------

_SHIM = {}


def shim_lib(tmp_root):
    """tests/series2_interval_oracle.cpp: the oracle's mul_rec<Interval> at rank 2 on plane-major buffers (built once per session)"""
    if "lib" not in _SHIM:
        so = os.path.join(str(tmp_root), "liborcis2.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so,
                               os.path.join(ROOT, "tests", "series2_interval_oracle.cpp")])
        L = C.CDLL(so)
        L.orci_series2_mul_raw.restype = C.c_int
        L.orci_series2_mul_raw.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t]
        _SHIM["lib"] = L
    return _SHIM["lib"]


@pytest.fixture(scope="session")
def shim2(tmp_path_factory):
    return shim_lib(tmp_path_factory.mktemp("orcis2"))


def data2(kind, B, shape, seed):
    """[2, B, n0, n1] interval items: the rows of test_interval_series_cpu.data over the row-major item ("pos", "mixed", "special": an
    exact [0,0] and one of [1,1], [-1,-1], an infinity, a NaN, [0,0] seeded past coefficient [0, 0], which stays in [0.5, 1.5))"""
    return data(kind, B, shape[0] * shape[1], seed).reshape((2, B) + tuple(shape))


def pad2i(a, n):
    """[2, s0, s1] (or fewer axes, as the oracle stores a constant) -> [2, n0, n1], +0 beyond"""
    a = np.asarray(a, dtype=np.float64)
    a = a.reshape(a.shape + (1,) * (3 - a.ndim))
    out = np.zeros((2,) + tuple(n))
    out[:, :a.shape[1], :a.shape[2]] = a
    return out


def mul_raw2(shim, x, y, n):
    """the shim on one item: x [2, nx0, nx1], y [2, ny0, ny1] -> [2, n0, n1]"""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    out = np.zeros((2,) + tuple(n))
    assert shim.orci_series2_mul_raw(C.c_void_p(x.ctypes.data), x.shape[1], x.shape[2], C.c_void_p(y.ctypes.data), y.shape[1], y.shape[2],
                                     C.c_void_p(out.ctypes.data), n[0], n[1]) == 0
    return out


def want_mul(shim, X, Y, n):
    return np.stack([mul_raw2(shim, X[:, b], Y[:, b], n) for b in range(X.shape[1])], axis=1)


def want_handle(OTPI, op, X, Y, n):
    """div / exp / log through the oracle's handle operators per item"""
    out = []
    for b in range(X.shape[1]):
        p = OTPI.new(X[:, b], n)
        r = p / OTPI.new(Y[:, b], n) if op == "div" else (p.exp() if op == "exp" else p.log())
        out.append(pad2i(r.array(), n))
    return np.stack(out, axis=1)


def is_normative(op, X, Y):
    """tests/_series2_oracle.oracle_is_normative: the divisor / the operand of log stores at least 2 coefficients on both axes"""
    t = Y if op == "div" else X
    return op in ("mul", "exp") or (t.shape[-2] >= 2 and t.shape[-1] >= 2)


def host_seeds(oracle_lib, op, X):
    """[2, B]: the interval exp / ln of coefficient [0, 0] per item"""
    return np.stack([scalar_fn(oracle_lib, op, X[:, b, 0, 0]) for b in range(X.shape[1])], axis=1)


def want_model(oracle_lib, op, X, Y, n, seeds=None):
    o = model.Ops(oracle_lib)
    out = []
    for b in range(X.shape[1]):
        if op in ("mul", "div"):
            out.append(getattr(model, op)(o, X[:, b], Y[:, b], n))
        else:
            sd = seeds[:, b] if seeds is not None else scalar_fn(oracle_lib, op, X[:, b, 0, 0])
            out.append(getattr(model, op)(o, X[:, b], n, sd))
    return np.stack(out, axis=1)


def _compact(a, b, n):
    return min(a.shape[1] + b.shape[1] - 1, n[0]), min(a.shape[2] + b.shape[2] - 1, n[1])


def chain_compose(shim, oracle_lib, f, g, var, n):
    """3.17's chain over intervals: Horner over the rows (var 0) or columns (var 1) of f, every product the shim's at the compact shape
    of the step, the slice add the oracle's scalar add"""
    f, g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
    nf0, nf1 = f.shape[1:]
    add = lambda a, b: scalar_add(oracle_lib, a, b)  # noqa: E731
    if var == 0:
        res = np.stack([add((0.0, 0.0), f[:, nf0 - 1, c]) for c in range(nf1)], axis=1).reshape(2, 1, nf1)
        for i in range(nf0 - 2, -1, -1):
            res = mul_raw2(shim, res, g, _compact(res, g, n))
            for c in range(nf1):
                res[:, 0, c] = add(res[:, 0, c], f[:, i, c])
    else:
        res = np.stack([add((0.0, 0.0), f[:, r, nf1 - 1]) for r in range(nf0)], axis=1).reshape(2, nf0, 1)
        for i in range(nf1 - 2, -1, -1):
            res = mul_raw2(shim, res, g, _compact(res, g, n))
            for r in range(nf0):
                res[:, r, 0] = add(res[:, r, 0], f[:, r, i])
    return pad2i(res, n)


def chain_pow(shim, x, e, n):
    """square-and-multiply without the last squaring, compact shapes, from [[[1,1]]]"""
    res, base = np.ones((2, 1, 1)), np.array(x, dtype=np.float64)
    while e > 0:
        if e & 1:
            res = mul_raw2(shim, res, base, _compact(res, base, n))
        e >>= 1
        if e > 0:
            base = mul_raw2(shim, base, base, _compact(base, base, n))
    return pad2i(res, n)


def want_compose(shim, oracle_lib, F, G, var, n):
    return np.stack([chain_compose(shim, oracle_lib, F[:, b], G[:, b], var, n) for b in range(F.shape[1])], axis=1)


def want_pow(shim, X, e, n):
    return np.stack([chain_pow(shim, X[:, b], e, n) for b in range(X.shape[1])], axis=1)


def bits_equal(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.where(np.isnan(want), np.isnan(got), got.view(np.int64) == want.view(np.int64))


def assert_bits(got, want, what):
    """every bit of every bound; where the expected bound is NaN, a NaN"""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    ok = bits_equal(got, want)
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {(~ok).sum()} bounds differ, first at {i}: got {got[i]!r} want {want[i]!r}")


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
    assert re.search(r"gfti_series2_pow\([^)]*uint32_t\s+e\b", header)
    assert re.search(r"gfti_series2_compose\([^)]*int\s+var\b", header)


def test_module_is_re_exported_and_shares_the_runner():
    import genfer_amd
    from genfer_amd import interval_series2, series2

    assert genfer_amd.interval_series2 is interval_series2
    for f in ("mul", "div", "exp", "log", "compose", "pow"):
        assert callable(getattr(interval_series2, f)) and getattr(interval_series2, f).__doc__
    from genfer_amd import _series_call, interval_series, series

    # one runner for every family and both ranks
    assert interval_series2._run is series2._run is series._run is interval_series._run is _series_call.run
    assert interval_series2.MAX_ELEMS == 2048 and series2.MAX_ELEMS == 4096


def test_python_side_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    from genfer_amd import interval_series2 as ivs2
    from genfer_amd.taylor import TaylorError

    d = _device_like(torch, (2, 3, 4, 8))
    # rank < 3: the plane axis and two series axes
    for bad in ((2, 8), (2,)):
        with pytest.raises(TaylorError, match="needs at least 3"):
            ivs2.mul(_device_like(torch, bad), d)
        with pytest.raises(TaylorError, match="y: .*needs at least 3"):
            ivs2.mul(d, _device_like(torch, bad))
    with pytest.raises(TaylorError, match=r"stacked \[2, \.\.\.\]"):
        ivs2.mul(_device_like(torch, (3, 3, 4, 8)), d)
    with pytest.raises(TaylorError, match=r"seed: .*stacked \[2, \.\.\.\]"):
        ivs2.exp(d, seed=_device_like(torch, (3,)))
    # an empty axis, a non-unit last stride
    for bad in ((2, 3, 0, 8), (2, 3, 4, 0)):
        with pytest.raises(TaylorError, match="a series axis is empty"):
            ivs2.exp(_device_like(torch, bad))
    with pytest.raises(TaylorError, match="unit stride"):
        ivs2.mul(_device_like(torch, (2, 3, 4, 16))[..., ::2], d)
    # the limit is 2048 coefficients; the f64 family keeps 4096
    big = _device_like(torch, (2, 1, 2, 8))
    for call in (lambda n: ivs2.mul(big, big, n=n), lambda n: ivs2.div(big, big, n=n), lambda n: ivs2.exp(big, n=n), lambda n: ivs2.log(big, n=n),
                 lambda n: ivs2.compose(big, big, 0, n=n), lambda n: ivs2.pow(big, 3, n=n)):
        with pytest.raises(TaylorError, match=r"= 2049 exceeds the limit of 2048"):
            call((3, 683))
        with pytest.raises(TaylorError, match="nx > n"):
            call((2, 7))
        with pytest.raises(TaylorError, match="n == 0"):
            call((0, 8))
    from genfer_amd import series2

    assert series2._orders("t", (64, 64), (1, 1)) == (64, 64)
    with pytest.raises(TaylorError, match="4096"):
        series2._orders("t", (17, 241), (1, 1))
    # var, the exponent
    for bad in (2, -1, 1.0, True, None):
        with pytest.raises(TaylorError, match="is 0 or 1"):
            ivs2.compose(d, d, var=bad)
    with pytest.raises(TaylorError, match="negative"):
        ivs2.pow(d, -1)
    with pytest.raises(TypeError, match="non-negative integer"):
        ivs2.pow(d, 2.5)
    # requires_grad: refused as in series2
    x = torch.zeros((2, 3, 4, 8), dtype=torch.float64, requires_grad=True)
    with pytest.raises(TaylorError, match="interval_series2 has no autograd"):
        ivs2.mul(x, x.detach())
    with pytest.raises(TaylorError, match="no autograd"):
        ivs2.exp(x)
    # out of the wrong shape
    with pytest.raises(TaylorError, match=r"out has \(4, 9\) coefficients per item"):
        ivs2.mul(d, d, out=_device_like(torch, (2, 3, 4, 9)))
    with pytest.raises(TaylorError, match="out has batch shape"):
        ivs2.mul(d, d, out=_device_like(torch, (2, 1, 4, 8)))
    with pytest.raises(TaylorError, match=r"out: .*stacked \[2, \.\.\.\]"):
        ivs2.mul(d, d, out=_device_like(torch, (1, 3, 4, 8)))
    # placement comes last
    with pytest.raises(TaylorError, match="on cpu"):
        ivs2.mul(x.detach(), x.detach())
    with pytest.raises(TaylorError, match="float32"):
        ivs2.mul(x.detach().float(), d)


def test_bench_series2_has_the_interval_mode():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_series2.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "--interval" in out.stdout


# ---- the gfx950 code ---------------------------------------------------------------------------------------------------------------


def test_series2_interval_isa(tmp_path):
    """The gfx950 code of the Interval<F64> instantiations (tests/series2_interval_isa_check.hip), what test_series2_isa asserts on the
    f64 code: no scratch in any kernel, no buffer instructions, no calls, separately rounded multiplies and adds.  The LDS layout is
    the interleaved one: an interval is one 16-byte element, read with ds_read_b128 in every kernel.  No FMA of any spelling and no
    division in mul and compose; div's FMAs are the five of each IEEE f64 division sequence (v_div_fmas_f64); exp and log have,
    besides those, exactly the FMAs of the device library's exp / log of their seed == NULL path (the file's two probe kernels)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function", "-Wno-pass-failed",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", "series2_interval_isa_check.hip")],
                          cwd=tmp_path)
    isa = open(glob.glob(str(tmp_path / "*amdgcn-amd-amdhsa*gfx950*.s"))[0]).read()
    # six interval kernels, the header's non-template f64 mul, two probes
    assert isa.count(".private_segment_fixed_size: 0") == 9 and isa.count(".private_segment_fixed_size:") == 9
    assert isa.count(".vgpr_spill_count: 0") == 9
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
    divs = lambda code: [c for c in code if c.startswith("v_div_") or c.startswith("v_rcp_f64")]  # noqa: E731
    mul = one("k_series2i_mul", "EIv")
    rec = {op: one("k_series2i_rec", f"EIvELi{op}E") for op in (1, 2, 3)}  # SERIES_DIV, _EXP, _LOG
    comp = [one("k_series2i_compose", "EIvELb1"), one("k_series2i_compose", "EIvELb0")]
    for code in [mul, rec[1], rec[2], rec[3]] + comp:
        assert not [c for c in code if c.startswith("scratch_") or c.startswith("buffer_")]
        assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")]
        assert any(c in ("ds_read_b128", "ds_load_b128") for c in code), "an interval in LDS is one 16-byte read"
        assert any(c in ("ds_write_b128", "ds_store_b128") for c in code)
        assert any(c.startswith("v_mul_f64") for c in code) and any(c.startswith("v_add_f64") for c in code)
    for code in [mul] + comp:
        assert fmas(code) == 0, "a contracted multiply-add"
        assert not divs(code)
        assert not [c for c in code if c.startswith("ds_read_b64") or c.startswith("ds_read2_b64")], "a bound read by itself"
    assert rec[1].count("v_div_fmas_f64") >= 1 and fmas(rec[1]) == 5 * rec[1].count("v_div_fmas_f64")
    probes = {log: [c for k, c in kernels.items() if "k_seed2_probe" in k and f"Lb{log}" in k] for log in (0, 1)}
    for log, code in ((0, rec[2]), (1, rec[3])):
        assert len(probes[log]) == 1 and probes[log][0].count("v_div_fmas_f64") == 0
        assert code.count("v_div_fmas_f64") >= 1
        assert fmas(code) == 5 * code.count("v_div_fmas_f64") + fmas(probes[log][0]), (log, fmas(code), fmas(probes[log][0]))


# ---- the expected values -----------------------------------------------------------------------------------------------------------

SHAPES = [(3, 3), (3, 5), (4, 7), (8, 8), (5, 16), (16, 5), (16, 16)]


def test_shim_product_equals_the_oracle_operator(OTPI, shim2):
    """on items with at least 3 stored coefficients on both axes of both factors the oracle's `*` takes none of its shortcuts (zero, one,
    constant, linear; mt:1014-1072) and runs mul_rec: the shim is that product"""
    for n in SHAPES:
        for xs, ys in [(n, n), tuple((max(3, s[0]), max(3, s[1])) for s in compact_shapes(*n))]:
            for kind in KINDS:
                X, Y = data2(kind, 3, xs, 100 * n[0] + n[1]), data2(kind, 3, ys, 200 * n[0] + n[1] + 1)
                want = np.stack([pad2i((OTPI.new(X[:, b], n) * OTPI.new(Y[:, b], n)).array(), n) for b in range(3)], axis=1)
                assert_bits(want_mul(shim2, X, Y, n), want, f"mul {n} x{xs} y{ys} {kind}")


def test_model_equals_the_shim_and_the_handle_operators(OTPI, oracle_lib, shim2):
    """the loops written out in scalar interval operations: the shim's product, and the oracle's `/`, exp() and log() where they are
    normative (the divisor / the operand of log stores at least 2 coefficients on both axes), special values included"""
    for n, xs, ys in [((2, 2), (2, 2), (2, 2)), ((3, 3), (3, 3), (3, 3)), ((3, 5), (3, 5), (3, 5)), ((4, 4), (2, 3), (3, 2)), ((3, 6), (3, 5), (2, 6))]:
        for kind in KINDS:
            X, Y = data2(kind, 2, xs, 300 * n[0] + n[1]), data2(kind, 2, ys, 400 * n[0] + n[1] + 3)
            assert_bits(want_model(oracle_lib, "mul", X, Y, n), want_mul(shim2, X, Y, n), f"model mul {n} {kind}")
            for op in ("div", "exp", "log"):
                assert is_normative(op, X, Y)
                assert_bits(want_model(oracle_lib, op, X, Y, n), want_handle(OTPI, op, X, Y, n), f"model {op} {n} x{xs} y{ys} {kind}")


def test_chains_equal_the_oracle_subst_var_and_pow(OTPI, shim2, oracle_lib):
    """for g with at least 3 stored coefficients on both axes the oracle's subst_var takes its general Horner path and every product
    the general one; pow likewise"""
    for n, fs, gs in [((3, 3), (3, 3), (3, 3)), ((4, 7), (4, 7), (3, 4)), ((8, 8), (8, 8), (8, 8)), ((5, 16), (2, 16), (5, 16)), ((16, 5), (16, 3), (9, 5)),
                      ((16, 16), (5, 9), (16, 16))]:
        for var in (0, 1):
            for kind in KINDS:
                F, G = data2(kind, 2, fs, 500 * n[0] + n[1] + var), data2(kind, 2, gs, 600 * n[0] + n[1] + 7)
                want = np.stack([pad2i(OTPI.new(F[:, b], n).subst_var(var, OTPI.new(G[:, b], n)).array(), n) for b in range(2)], axis=1)
                assert_bits(want_compose(shim2, oracle_lib, F, G, var, n), want, f"compose var={var} {n} f{fs} g{gs} {kind}")
    for n, xs in [((3, 3), (3, 3)), ((8, 8), (8, 8)), ((5, 16), (3, 9)), ((16, 16), (16, 16))]:
        for kind in KINDS:
            X = data2(kind, 2, xs, 700 * n[0] + n[1])
            for e in (2, 3, 5, 8):
                want = np.stack([pad2i(OTPI.new(X[:, b], n).pow(e).array(), n) for b in range(2)], axis=1)
                assert_bits(want_pow(shim2, X, e, n), want, f"pow {n} x{xs} e={e} {kind}")
