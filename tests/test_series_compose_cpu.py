"""Batched compose and pow (genfer_amd.series.compose / pow, gft_series_compose / gft_series_pow) without a GPU: the exported and
declared surface, the refusals the Python side makes before it touches the library, the gfx950 code of the two compose kernels,
and the definition itself — the chain of general products built from orc_mul_raw against the oracle's subst_var / pow on the
dense inputs the GPU tests use (tests/test_series_compose_gpu.py imports the cases and the chains from this file)."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, splitmix64_uniform

SYMBOLS = ("gft_series_compose", "gft_series_pow")

# ---- the cases and the expected values shared with the GPU tests ------------------------------------------------------------

ORDERS = [1, 2, 3, 7, 16, 31, 32, 33, 64, 65, 100, 257, 1024, 4096]
BATCHES = [1, 3, 64, 65, 1000]
CPU_BUDGET = 7.0e7  # B * nf * n^2 per case: the oracle side stays within seconds
POW_E = [0, 1, 2, 3, 5, 8, 13, 31, 64]
POW_SHAPES = [(16, 16, 1000), (40, 40, 65), (40, 9, 65), (100, 100, 3), (100, 3, 3), (300, 300, 64), (300, 1, 3)]  # (n, nx, B)


def dense(shape, seed):
    """0.5 + uniform: dense rows on which the oracle's operators take no shortcut"""
    return (0.5 + splitmix64_uniform(seed, int(np.prod(shape)))).reshape(shape)


def pad(a, n):
    out = np.zeros(n)
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    out[:a.size] = a
    return out


def compose_lengths(n, B):
    """(nf, ng) within the CPU budget: dense, the compact corners nf = 1, nf = 2, ng = 1, ng = 2 (with ng = n on the f side), two
    halves, and where the dense pair is beyond the budget the longest f that fits it against a dense g"""
    cand = [(n, n), (1, n), (2, n), (n, 1), (n, 2), (n // 2 + 1, n // 2 + 2)]
    top = int(CPU_BUDGET // (B * n * n))
    if top < n:
        cand.append((top, n))
    out = []
    for nf, ng in cand:
        if 1 <= nf <= n and 1 <= ng <= n and B * nf * n * n <= CPU_BUDGET and (nf, ng) not in out:
            out.append((nf, ng))
    return out


def compose_cases():
    """(n, B, nf, ng): every order, every batch size the budget allows; the compact corners on two of the batch sizes"""
    for n in ORDERS:
        for B in BATCHES:
            for k, (nf, ng) in enumerate(compose_lengths(n, B)):
                if k > 0 and (nf, ng) != (n, n) and B not in (3, 65) and not (n >= 1024 and B == 1):
                    continue
                yield n, B, nf, ng


def compose_inputs(n, B, nf, ng):
    return dense((B, nf), 3000 * n + 17 * B + nf), dense((B, ng), 5000 * n + 13 * B + ng + 7)


def mul_raw(oracle_lib, x, y, n):
    """orc_mul_raw on a zeroed result: mul_1d, z[k] = 0.0 + sum_j x[j] * y[k-j] in ascending j, no dispatcher"""
    szp = C.POINTER(C.c_size_t)
    oracle_lib.orc_mul_raw.restype = C.c_int
    oracle_lib.orc_mul_raw.argtypes = [C.c_void_p, szp, C.c_void_p, szp, C.c_void_p, szp, C.c_size_t]
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    out = np.zeros(n)
    one = lambda v: (C.c_size_t * 1)(v)  # noqa: E731
    assert oracle_lib.orc_mul_raw(x.ctypes.data_as(C.c_void_p), one(x.size), y.ctypes.data_as(C.c_void_p), one(y.size),
                                  out.ctypes.data_as(C.c_void_p), one(n), 1) == 0
    return out


def chain_compose(oracle_lib, f, g, n):
    """the definition: Horner over f with the general product at the compact length of every step"""
    with np.errstate(all="ignore"):
        res = np.array([0.0 + f[-1]])
        for i in range(f.size - 2, -1, -1):
            res = mul_raw(oracle_lib, res, g, min(res.size + g.size - 1, n))
            res[0] = res[0] + f[i]
    return pad(res, n)


def chain_pow(oracle_lib, x, e, n):
    """the definition: square-and-multiply without the last squaring, compact lengths"""
    with np.errstate(all="ignore"):
        res, base = np.array([1.0]), np.array(x, dtype=np.float64)
        while e > 0:
            if e & 1:
                res = mul_raw(oracle_lib, res, base, min(res.size + base.size - 1, n))
            e >>= 1
            if e > 0:
                base = mul_raw(oracle_lib, base, base, min(2 * base.size - 1, n))
    return pad(res, n)


def want_compose(oracle_lib, F, G, n):
    return np.stack([chain_compose(oracle_lib, F[b], G[b], n) for b in range(F.shape[0])])


def want_pow(oracle_lib, X, e, n):
    return np.stack([chain_pow(oracle_lib, X[b], e, n) for b in range(X.shape[0])])


def oracle_compose(OTP, F, G, n):
    return np.stack([pad(OTP.new(F[b], (n,)).subst_var(0, OTP.new(G[b], (n,))).array(), n) for b in range(F.shape[0])])


def oracle_pow(OTP, X, e, n):
    return np.stack([pad(OTP.new(X[b], (n,)).pow(e).array(), n) for b in range(X.shape[0])])


def same_bits(a, b):
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
    assert re.search(r"gft_series_pow\([^)]*uint32_t\s+e\b", header)
    assert "e: u32" in [ln for ln in doc.splitlines() if "pub fn gft_series_pow(" in ln][0]


def test_module_has_compose_and_pow():
    from genfer_amd import series

    assert callable(series.compose) and callable(series.pow)
    assert "compose" in series.__doc__ and "pow" in series.__doc__
    assert "nf * n**2 / 2" in series.compose.__doc__  # the cost is stated where a caller reads it


def test_python_side_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    x = torch.zeros((3, 8), dtype=torch.float64)
    with pytest.raises(TaylorError, match="f: .*on cpu"):
        series.compose(x, x)
    with pytest.raises(TaylorError, match="on cpu"):
        series.pow(x, 2)
    with pytest.raises(TaylorError, match="f: .*float32"):
        series.compose(x.float(), x)
    with pytest.raises(TaylorError, match="float32"):
        series.pow(x.float(), 2)
    with pytest.raises(TypeError, match="torch.Tensor"):
        series.compose([1.0, 2.0], x)
    with pytest.raises(TaylorError, match="g: .*on cpu"):
        series.compose(_device_like(torch, (3, 8)), x)
    # the exponent is judged before anything else
    with pytest.raises(TaylorError, match="negative"):
        series.pow(x, -1)
    for bad in (2.5, 2.0, "3", None, True):
        with pytest.raises(TypeError, match="non-negative integer"):
            series.pow(x, bad)
    with pytest.raises(TaylorError, match="32 bits"):
        series.pow(x, 2**32)


def _device_like(torch, shape):
    """a tensor without storage (meta) that reports a GPU placement: it passes the placement check, so the checks behind it
    (the second operand, the orders) are reached without a device"""

    class Fake(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)

    return torch.zeros(shape, dtype=torch.float64, device="meta").as_subclass(Fake)


def test_order_checks():
    """nf > n, n == 0 and n > 4096 are refused by the checks compose and pow share with the other operations"""
    torch = pytest.importorskip("torch")
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    f, g = _device_like(torch, (3, 8)), _device_like(torch, (3, 5))
    with pytest.raises(TaylorError, match="nx > n"):
        series.compose(f, g, n=6)
    with pytest.raises(TaylorError, match="nx > n"):
        series.compose(g, f, n=6)
    with pytest.raises(TaylorError, match="n == 0"):
        series.compose(f, g, n=0)
    with pytest.raises(TaylorError, match="4096"):
        series.compose(f, g, n=4097)
    with pytest.raises(TaylorError, match="nx > n"):
        series.pow(f, 3, n=4)
    with pytest.raises(TaylorError, match="n == 0"):
        series.pow(f, 3, n=0)
    with pytest.raises(TaylorError, match="4096"):
        series.pow(f, 3, n=4097)


def test_bench_series_knows_the_new_operations():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_series", os.path.join(ROOT, "tools", "bench_series.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse_args(["--ops", "compose,pow"])
    assert args.ops == "compose,pow"
    assert "compose" in mod.KNOWN_OPS and "pow" in mod.KNOWN_OPS


# ---- the gfx950 code ---------------------------------------------------------------------------------------------------------------


def test_compose_isa(tmp_path):
    """The gfx950 code of the two compose kernels (tests/series_compose_isa_check.hip): no scratch, no calls, no buffer
    instructions, LDS reads, separately rounded v_mul_f64 / v_add_f64 and no FMA of any spelling (compose has no division)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", "series_compose_isa_check.hip")],
                          cwd=tmp_path)
    isa = open(glob.glob(str(tmp_path / "*amdgcn-amd-amdhsa*gfx950*.s"))[0]).read()
    assert isa.count(".private_segment_fixed_size: 0") == 2 and isa.count(".private_segment_fixed_size:") == 2
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
    a = [c for k, c in kernels.items() if "k_series_compose_a" in k]
    b = [c for k, c in kernels.items() if "k_series_compose_b" in k]
    assert len(a) == 1 and len(b) == 1 and len(a[0]) > 50 and len(b[0]) > 50
    for code in (a[0], b[0]):
        assert not [c for c in code if c.startswith("scratch_") or c.startswith("buffer_")]
        assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")]
        assert any(c.startswith("ds_read") or c.startswith("ds_load") for c in code)
        assert any(c.startswith("v_mul_f64") for c in code) and any(c.startswith("v_add_f64") for c in code)
        assert not [c for c in code if "fma" in c or c.startswith("v_fmac") or c.startswith("v_mad_f64")], "a contracted multiply-add"
        assert not [c for c in code if c.startswith("v_div_") or c.startswith("v_rcp_f64")]
    assert any(c == "s_barrier" for c in b[0])  # the steps of form B meet at a barrier


# ---- the definition ----------------------------------------------------------------------------------------------------------------

ROWS = 3  # rows of every case compared here (the GPU tests compare all of them)


def test_chain_equals_the_oracle_subst_var(OTP, oracle_lib):
    """for dense data and ng >= 3 the oracle's subst_var takes its general Horner path and every product the general mul_1d: the
    chain the GPU tests use as expected value for the other cases is the same function"""
    seen = 0
    for n, B, nf, ng in compose_cases():
        if ng < 3:
            continue
        F, G = compose_inputs(n, B, nf, ng)
        F, G = F[:ROWS], G[:ROWS]
        assert same_bits(want_compose(oracle_lib, F, G, n), oracle_compose(OTP, F, G, n)), (n, B, nf, ng)
        seen += 1
    assert seen >= 40


def test_chain_is_the_written_definition(oracle_lib):
    """the chain against the loops of the definition written out in numpy scalars (ng <= 2 and specials included, where the
    oracle's operators would shortcut)"""
    inf, nan = float("inf"), float("nan")
    cases = [([1.5, -2.0, 0.25], [0.5, 3.0], 6), ([2.0], [1.0, 2.0, 3.0], 4), ([1.0, 2.0, 3.0, 4.0], [0.75], 5),
             ([0.0, 1.0, -0.0, 2.0], [0.0, 1.0, 0.0], 7), ([1.0, inf, 2.0], [0.5, nan, 1.0], 5), ([-0.0], [1.0], 3),
             ([1.0, 1.0, 1.0], [0.0, 0.0, inf], 9)]
    for f, g, n in cases:
        f, g = np.array(f), np.array(g)
        with np.errstate(all="ignore"):
            res = [0.0 + f[-1]]
            for i in range(f.size - 2, -1, -1):
                L = min(len(res) + g.size - 1, n)
                new = []
                for k in range(L):
                    s = np.float64(0.0)
                    for j in range(max(0, k + 1 - g.size), min(k + 1, len(res))):
                        s = s + np.float64(res[j]) * g[k - j]
                    new.append(s)
                new[0] = new[0] + f[i]
                res = new
        assert same_bits(chain_compose(oracle_lib, f, g, n), pad(res, n)), (f, g, n)


def test_chain_equals_the_oracle_pow(OTP, oracle_lib):
    for n, nx, B in POW_SHAPES:
        X = dense((B, nx), 700 * n + nx)[:ROWS]
        for e in POW_E:
            assert same_bits(want_pow(oracle_lib, X, e, n), oracle_pow(OTP, X, e, n)), (n, nx, e)
