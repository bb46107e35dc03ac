"""Batched interval series (genfer_amd.interval_series, gfti_series_*) without a GPU: the exported and declared surface, the
refusals the Python side makes before it touches the library, the measurement tool's command line, the gfx950 code of the
Interval<F64> instantiations of the series kernels, and the expected values themselves -- the raw interval product of
tests/series_interval_oracle.cpp against the oracle's operator, and the compose / pow chains built over it against the oracle's
subst_var / pow and against the loops written out in scalar interval operations (tests/test_interval_series_gpu.py imports the
data, the cases and the expected values from this file)."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, splitmix64_uniform

SYMBOLS = ("gfti_series_mul", "gfti_series_div", "gfti_series_exp", "gfti_series_log", "gfti_series_compose", "gfti_series_pow")
INF, NAN = float("inf"), float("nan")

# ---- the expected values shared with the GPU tests ----------------------------------------------------------------------------

_SHIM = {}


def shim_lib(tmp_root):
    """tests/series_interval_oracle.cpp: the oracle's mul_rec<Interval> on plane-major buffers (built once per session)"""
    if "lib" not in _SHIM:
        so = os.path.join(str(tmp_root), "liborcis.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so,
                               os.path.join(ROOT, "tests", "series_interval_oracle.cpp")])
        L = C.CDLL(so)
        L.orci_series_mul_raw.restype = C.c_int
        L.orci_series_mul_raw.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        _SHIM["lib"] = L
    return _SHIM["lib"]


@pytest.fixture(scope="session")
def shim(tmp_path_factory):
    return shim_lib(tmp_path_factory.mktemp("orcis"))


def scalar_op(oracle_lib, code, a, b=None):
    """one scalar operation of the oracle's Interval (orci_scalar_op: 0 add, 2 mul, 5 exp, 6 log).  Plain double[2] arguments: they
    serve the function with or without the argtypes another test module may have declared on it"""
    D2 = C.c_double * 2
    out = D2()
    assert oracle_lib.orci_scalar_op(code, D2(float(a[0]), float(a[1])), None if b is None else D2(float(b[0]), float(b[1])), out) == 0
    return np.array(out[:])


def scalar_add(oracle_lib, a, b):
    """the oracle's scalar interval add (iv:126-139)"""
    return scalar_op(oracle_lib, 0, a, b)


def scalar_fn(oracle_lib, op, a):
    """the oracle's scalar interval exp / log: the seeds a host can form (platform libm, widened)"""
    return scalar_op(oracle_lib, {"exp": 5, "log": 6}[op], a)


def data(kind, B, n, seed):
    """[2, B, n] interval rows.  "pos": 0 < lo <= hi, about 2^-20 wide.  "mixed": both signs and about 2^-10 wide from
    coefficient 1 on (some straddle zero); coefficient 0, which div divides by and log takes the logarithm of, stays in
    [0.5, 1.5).  "special": the mixed rows, each seeded at a coefficient >= 1 with an exact [0,0] and one of [1,1], [-1,-1],
    [lo, inf], [nan, nan], [0,0] (the short-circuits of interval.rs:126-234 and what they must not swallow)."""
    u = splitmix64_uniform(seed, 2 * B * n).reshape(2, B, n)
    lo = 0.5 + u[0]
    if kind == "pos":
        return np.stack([lo, lo + u[1] * 2.0**-20])
    c = 3.0 * u[0] - 1.5
    c[:, 0] = lo[:, 0]
    out = np.stack([c, c + u[1] * 2.0**-10])
    if kind == "special" and n >= 2:
        kinds = [(1.0, 1.0), (-1.0, -1.0), (None, INF), (NAN, NAN), (0.0, 0.0)]
        for b in range(B):
            k = 1 + (b // len(kinds)) % (n - 1)
            l, h = kinds[b % len(kinds)]
            out[:, b, k] = (out[0, b, k] if l is None else l, h)
            z = 1 + (k + 1 + b) % (n - 1)
            if z != k:
                out[:, b, z] = 0.0
    return out


def pad(a, n):
    """[2, len] -> [2, n], +0 beyond"""
    a = np.asarray(a, dtype=np.float64).reshape(2, -1)
    out = np.zeros((2, n))
    out[:, :a.shape[1]] = a
    return out


def mul_raw(shim, x, y, n):
    """the shim on one item: x [2, nx], y [2, ny] -> [2, n]"""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    out = np.zeros((2, n))
    assert shim.orci_series_mul_raw(C.c_void_p(x.ctypes.data), x.shape[1], C.c_void_p(y.ctypes.data), y.shape[1],
                                    C.c_void_p(out.ctypes.data), n) == 0
    return out


def want_mul(shim, X, Y, n):
    return np.stack([mul_raw(shim, X[:, b], Y[:, b], n) for b in range(X.shape[1])], axis=1)


def want_handle(OTPI, op, X, Y, n):
    """div / exp / log through the oracle's handle operators per item; the divisor and the operand of exp / log hold at least two
    coefficients, so the operators take their general paths (their shortcuts look at the stored length, mt:1204-1213)"""
    assert (Y if op == "div" else X).shape[2] >= 2
    out = []
    for b in range(X.shape[1]):
        p = OTPI.new(X[:, b], (n,))
        r = p / OTPI.new(Y[:, b], (n,)) if op == "div" else (p.exp() if op == "exp" else p.log())
        out.append(pad(r.array(), n))
    return np.stack(out, axis=1)


def host_seeds(oracle_lib, op, X):
    """[2, B]: the interval exp / ln of coefficient 0 per item"""
    return np.stack([scalar_fn(oracle_lib, op, X[:, b, 0]) for b in range(X.shape[1])], axis=1)


def chain_compose(shim, oracle_lib, f, g, n):
    """the definition (tests/test_series_compose_cpu.py's chain over intervals): Horner over f with the general product at the compact
    length of every step and the oracle's scalar add"""
    res = scalar_add(oracle_lib, (0.0, 0.0), f[:, -1]).reshape(2, 1)
    for i in range(f.shape[1] - 2, -1, -1):
        res = mul_raw(shim, res, g, min(res.shape[1] + g.shape[1] - 1, n))
        res[:, 0] = scalar_add(oracle_lib, res[:, 0], f[:, i])
    return pad(res, n)


def chain_pow(shim, x, e, n):
    """the definition: square-and-multiply without the last squaring, compact lengths"""
    res, base = np.array([[1.0], [1.0]]), np.array(x, dtype=np.float64)
    while e > 0:
        if e & 1:
            res = mul_raw(shim, res, base, min(res.shape[1] + base.shape[1] - 1, n))
        e >>= 1
        if e > 0:
            base = mul_raw(shim, base, base, min(2 * base.shape[1] - 1, n))
    return pad(res, n)


def want_compose(shim, oracle_lib, F, G, n):
    return np.stack([chain_compose(shim, oracle_lib, F[:, b], G[:, b], n) for b in range(F.shape[1])], axis=1)


def want_pow(shim, X, e, n):
    return np.stack([chain_pow(shim, X[:, b], e, n) for b in range(X.shape[1])], axis=1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all(np.where(np.isnan(b), np.isnan(a), a.view(np.int64) == b.view(np.int64))))


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
    assert re.search(r"gfti_series_pow\([^)]*uint32_t\s+e\b", header)
    from genfer_amd.taylor import HANDLE_API

    assert not [n for n in HANDLE_API if n.startswith("series")]  # raw entry points, not handle operators


def test_module_is_re_exported_and_shares_the_runner():
    import genfer_amd
    from genfer_amd import interval_series, series

    assert genfer_amd.interval_series is interval_series
    for f in ("mul", "div", "exp", "log", "compose", "pow"):
        assert callable(getattr(interval_series, f)) and getattr(interval_series, f).__doc__
    from genfer_amd import _series_call, interval_series2, series2

    # one runner for every family and both ranks
    assert interval_series._run is series._run is series2._run is interval_series2._run is _series_call.run
    assert interval_series.last_form is series.last_form and interval_series.set_form is series.set_form
    assert interval_series.MAX_N == 2048 and series.MAX_N == 4096


def _device_like(torch, shape):
    """a tensor without storage (meta) that reports a GPU placement: it passes the placement check, so the checks behind it are
    reached without a device"""

    class Fake(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)

    return torch.zeros(shape, dtype=torch.float64, device="meta").as_subclass(Fake)


def test_python_side_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    from genfer_amd import interval_series as ivs
    from genfer_amd.taylor import TaylorError

    x = torch.zeros((2, 3, 8), dtype=torch.float64)
    for f in (ivs.mul, ivs.div, ivs.compose):
        with pytest.raises(TaylorError, match="on cpu"):
            f(x, x)
        with pytest.raises(TaylorError, match="float32"):
            f(x.float(), x)
    for f in (ivs.exp, ivs.log, lambda t: ivs.pow(t, 2)):
        with pytest.raises(TaylorError, match="on cpu"):
            f(x)
        with pytest.raises(TaylorError, match="float32"):
            f(x.float())
    with pytest.raises(TypeError, match="torch.Tensor"):
        ivs.mul([1.0, 2.0], x)
    with pytest.raises(TaylorError, match="g: .*on cpu"):
        ivs.compose(_device_like(torch, (2, 3, 8)), x)
    # the first axis holds the two planes
    d = _device_like(torch, (2, 3, 8))
    for bad in ((3, 3, 8), (1, 3, 8), (3, 8)):
        with pytest.raises(TaylorError, match=r"stacked \[2, \.\.\.\]"):
            ivs.mul(_device_like(torch, bad), d)
        with pytest.raises(TaylorError, match=r"y: .*stacked \[2, \.\.\.\]"):
            ivs.mul(d, _device_like(torch, bad))
    with pytest.raises(TaylorError, match=r"seed: .*stacked \[2, \.\.\.\]"):
        ivs.exp(d, seed=_device_like(torch, (3,)))
    with pytest.raises(TaylorError, match="no series axis"):
        ivs.mul(_device_like(torch, (2,)), d)
    with pytest.raises(TaylorError, match="unit stride"):
        ivs.mul(_device_like(torch, (2, 3, 16))[..., ::2], d)
    # the exponent is judged before anything else
    with pytest.raises(TaylorError, match="negative"):
        ivs.pow(x, -1)
    for bad in (2.5, "3", None, True):
        with pytest.raises(TypeError, match="non-negative integer"):
            ivs.pow(x, bad)
    with pytest.raises(TaylorError, match="32 bits"):
        ivs.pow(x, 2**32)


def test_order_checks():
    torch = pytest.importorskip("torch")
    from genfer_amd import interval_series as ivs
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    f, g = _device_like(torch, (2, 3, 8)), _device_like(torch, (2, 3, 5))
    for call in (lambda n: ivs.mul(f, g, n=n), lambda n: ivs.div(g, f, n=n), lambda n: ivs.compose(f, g, n=n), lambda n: ivs.exp(f, n=n),
                 lambda n: ivs.log(f, n=n), lambda n: ivs.pow(f, 3, n=n)):
        with pytest.raises(TaylorError, match="nx > n"):
            call(6)
        with pytest.raises(TaylorError, match="n == 0"):
            call(0)
        with pytest.raises(TaylorError, match="2048"):
            call(2049)
    # the f64 family keeps its own limit
    assert series._order("t", 4096, 1) == 4096
    with pytest.raises(TaylorError, match="4096"):
        series._order("t", 4097, 8)


def test_bench_series_has_the_interval_mode():
    import importlib.util

    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_series.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "--interval" in out.stdout and "--form" in out.stdout and "--ops" in out.stdout
    spec = importlib.util.spec_from_file_location("bench_series", os.path.join(ROOT, "tools", "bench_series.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["--ops", "compose,pow"]).ops == "compose,pow"
    assert mod.parse_args(["--interval"]).interval and not mod.parse_args([]).interval


# ---- the gfx950 code ---------------------------------------------------------------------------------------------------------------


def test_interval_series_isa(tmp_path):
    """The gfx950 code of the Interval<F64> instantiations (tests/series_interval_isa_check.hip): no scratch in any kernel (an
    interval multiply-add keeps many values live; a spill would show here), no buffer instructions, no calls, LDS reads,
    separately rounded multiplies and adds.  No FMA of any spelling and no division in the mul and compose kernels; the div
    kernel's FMAs are the five of each IEEE f64 division sequence (v_div_fmas_f64); the exp / log kernels have, besides those,
    exactly the FMAs of the device library's exp / log of their seed == NULL path, counted on the file's two probe kernels."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", "series_interval_isa_check.hip")],
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
    divs = lambda code: [c for c in code if c.startswith("v_div_") or c.startswith("v_rcp_f64")]  # noqa: E731
    mul_a, div_a, compose_a = one("k_series_mul_a", "EIv"), one("k_series_div_a", "EIv"), one("k_series_compose_a", "EIv")
    exp_a, log_a = one("k_series_explog_a", "EIvELb0"), one("k_series_explog_a", "EIvELb1")
    mul_b, compose_b = one("k_series_mul_b", "EIv"), one("k_series_compose_b", "EIvELb1")
    for code in (mul_a, div_a, compose_a, exp_a, log_a, mul_b, compose_b):
        assert not [c for c in code if c.startswith("scratch_") or c.startswith("buffer_")]
        assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")]
        assert any(c.startswith("ds_read") or c.startswith("ds_load") for c in code)
        assert any(c.startswith("v_mul_f64") for c in code) and any(c.startswith("v_add_f64") for c in code)
    for code in (mul_a, compose_a, mul_b, compose_b):
        assert fmas(code) == 0, "a contracted multiply-add"
        assert not divs(code)
    assert any(c == "s_barrier" for c in compose_b)
    assert div_a.count("v_div_fmas_f64") >= 1 and fmas(div_a) == 5 * div_a.count("v_div_fmas_f64")
    probes = {log: [c for k, c in kernels.items() if "k_seed_probe" in k and f"Lb{log}" in k] for log in (0, 1)}
    for log, code in ((0, exp_a), (1, log_a)):
        assert len(probes[log]) == 1 and probes[log][0].count("v_div_fmas_f64") == 0  # (the library's log has a v_rcp_f64 of its own)
        assert code.count("v_div_fmas_f64") >= 1
        assert fmas(code) == 5 * code.count("v_div_fmas_f64") + fmas(probes[log][0]), (log, fmas(code), fmas(probes[log][0]))


# ---- the expected values -----------------------------------------------------------------------------------------------------------

SHAPES = [(3, 3, 3), (7, 4, 7), (16, 16, 16), (33, 20, 33), (64, 64, 40), (100, 100, 100), (257, 130, 257)]  # (n, nx, ny)
KINDS = ("pos", "mixed", "special")


def test_shim_product_equals_the_oracle_operator(OTPI, shim):
    """on rows with both lengths >= 3 the oracle's `*` takes none of its shortcuts (they look at the stored shapes: zero, one,
    constant, linear; mt:1014-1072) and runs mul_rec: the shim is that product"""
    for n, nx, ny in SHAPES:
        for kind in KINDS:
            X, Y = data(kind, 3, nx, 100 * n + nx), data(kind, 3, ny, 200 * n + ny + 1)
            want = np.stack([pad((OTPI.new(X[:, b], (n,)) * OTPI.new(Y[:, b], (n,))).array(), n) for b in range(3)], axis=1)
            assert same_bits(want_mul(shim, X, Y, n), want), (n, nx, ny, kind)


def test_chains_equal_the_oracle_subst_var_and_pow(OTPI, shim, oracle_lib):
    """for ng >= 3 the oracle's subst_var takes its general Horner path and every product the general one; pow likewise"""
    for n, nf, ng in [(3, 3, 3), (7, 5, 4), (16, 16, 16), (33, 9, 33), (40, 40, 3), (64, 2, 64), (64, 1, 5), (100, 30, 100)]:
        for kind in KINDS:
            F, G = data(kind, 3, nf, 300 * n + nf), data(kind, 3, ng, 500 * n + ng + 7)
            want = np.stack([pad(OTPI.new(F[:, b], (n,)).subst_var(0, OTPI.new(G[:, b], (n,))).array(), n) for b in range(3)], axis=1)
            assert same_bits(want_compose(shim, oracle_lib, F, G, n), want), ("compose", n, nf, ng, kind)
    for n, nx in [(16, 16), (40, 9), (100, 3), (64, 64)]:
        for kind in KINDS:
            X = data(kind, 3, nx, 700 * n + nx)
            for e in (2, 3, 5, 8, 13):
                want = np.stack([pad(OTPI.new(X[:, b], (n,)).pow(e).array(), n) for b in range(3)], axis=1)
                assert same_bits(want_pow(shim, X, e, n), want), ("pow", n, nx, e, kind)


def test_chain_is_the_written_definition(shim, oracle_lib):
    """the compose chain against the loops of the definition written out in scalar interval operations (orci_scalar_op), exact
    zeros, [1,1], an infinity and a NaN included, ng <= 2 too (where the oracle's operators would shortcut)"""

    op = lambda code, a, b: scalar_op(oracle_lib, code, a, b)  # noqa: E731

    iv = lambda *pairs: np.array(pairs, dtype=np.float64).T  # noqa: E731  ([2, len])
    cases = [(iv((1.5, 1.6), (-2.0, -1.9), (0.25, 0.25)), iv((0.5, 0.5), (3.0, 3.5)), 6),
             (iv((2.0, 2.5)), iv((1.0, 1.0), (2.0, 2.0), (3.0, 3.0)), 4),
             (iv((1.0, 1.0), (2.0, 2.1), (3.0, 3.0), (4.0, 4.0)), iv((0.75, 0.75)), 5),
             (iv((0.0, 0.0), (1.0, 1.0), (0.0, 0.0), (2.0, 2.0)), iv((0.0, 0.0), (1.0, 1.0), (0.0, 0.0)), 7),
             (iv((1.0, 1.0), (1.0, INF), (2.0, 2.0)), iv((0.5, 0.5), (NAN, NAN), (1.0, 1.0)), 5),
             (iv((-1.0, -1.0), (0.0, 0.0), (1.0, 1.0)), iv((-0.5, 0.5), (0.0, 0.0), (-INF, 1.0)), 9),
             (iv((1.0, 1.0), (1.0, 1.0), (1.0, 1.0)), iv((0.0, 0.0), (0.0, 0.0), (2.0, INF)), 9)]
    for f, g, n in cases:
        nf, ng = f.shape[1], g.shape[1]
        res = [op(0, (0.0, 0.0), f[:, nf - 1])]
        for i in range(nf - 2, -1, -1):
            L = min(len(res) + ng - 1, n)
            new = []
            for k in range(L):
                s = np.zeros(2)
                for j in range(max(0, k + 1 - ng), min(k + 1, len(res))):
                    s = op(0, s, op(2, res[j], g[:, k - j]))
                new.append(s)
            new[0] = op(0, new[0], f[:, i])
            res = new
        assert same_bits(chain_compose(shim, oracle_lib, f, g, n), pad(np.array(res).T, n)), (f, g, n)



# ---- the cost of the expected values ---------------------------------------------------------------------------------------------


def test_oracle_side_stays_within_the_f64_files(OTP, OTPI, oracle_lib, shim):
    """every expected value tests/test_interval_series_gpu.py asks the oracle for takes no more CPU time than the bit-exact loops of
    the two f64 files (tests/test_series_batch_gpu.py: mul / div / exp / log; tests/test_series_compose_gpu.py: compose and pow) --
    both timed here, one after the other on this host.  The figures of the development host are written at CPU_BUDGET there."""
    import time

    import test_interval_series_gpu as ig
    import test_series_batch_gpu as bg
    import test_series_compose_cpu as cc

    t0 = time.time()
    with np.errstate(all="ignore"):
        for op in ("mul", "div", "exp", "log"):
            for n, B in bg.cases():
                for nx, ny in bg.lengths(op, n, B):
                    x, y = bg.dense((B, nx), 1000 * n + B), bg.dense((B, ny), 2000 * n + B + 7)
                    bg.want_mul(oracle_lib, x, y, n) if op == "mul" else bg.want_handle(OTP, op, x, y, n)
        t_batch = time.time() - t0
        for n, B, nf, ng in cc.compose_cases():
            F, G = cc.compose_inputs(n, B, nf, ng)
            cc.oracle_compose(OTP, F, G, n) if ng >= 3 else cc.want_compose(oracle_lib, F, G, n)
        t_compose = time.time() - t0 - t_batch
        for n, nx, B in cc.POW_SHAPES:
            x = cc.dense((B, nx), 900 * n + nx)
            for e in cc.POW_E:
                cc.oracle_pow(OTP, x, e, n), cc.want_pow(oracle_lib, x, e, n)
    f64 = time.time() - t0
    took = ig.oracle_side_seconds(OTPI, oracle_lib, shim)
    print(f"f64 files: {f64:.1f} s (batch {t_batch:.1f}, compose {t_compose:.1f}, pow {f64 - t_batch - t_compose:.1f}); interval file: "
          f"{sum(took.values()):.1f} s ({', '.join(f'{k} {v:.1f}' for k, v in took.items())})")
    assert sum(took.values()) <= f64, (took, f64)
