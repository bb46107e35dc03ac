"""Batched bivariate compose and pow (genfer_amd.series2.compose / pow, gft_series2_compose / gft_series2_pow) without a GPU: the
exported and declared surface, the refusals the Python side makes before it touches a device, the definition itself -- the chains
of general products built from orc_mul_raw at rank 2 against the oracle's subst_var / pow and against the plain-Python model --
the measurement tool's command line, and the gfx950 code of both instantiations of the compose kernel."""
import glob
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _series2_compose_cases as cc
from _series2_oracle import bits_equal, dense
from conftest import ROOT

SYMBOLS = ("gft_series2_compose", "gft_series2_pow")


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
    assert re.search(r"gft_series2_pow\([^)]*uint32_t\s+e\b", header)
    assert re.search(r"gft_series2_compose\([^)]*\bint\s+var\b", header)
    assert "e: u32" in [ln for ln in doc.splitlines() if "pub fn gft_series2_pow(" in ln][0]
    assert "var: c_int" in [ln for ln in doc.splitlines() if "pub fn gft_series2_compose(" in ln][0]


def test_module_has_compose_and_pow():
    from genfer_amd import series2

    assert callable(series2.compose) and callable(series2.pow)
    assert "compose" in series2.__doc__ and "pow" in series2.__doc__
    assert "no ``compose``" not in series2.__doc__
    assert "nslices * (n0*n1)**2 / 4" in series2.compose.__doc__ and "no cap" in series2.compose.__doc__  # the cost, where a caller reads it
    assert series2.pow.__doc__


def _device_like(torch, shape):
    """a tensor without storage (meta) that reports a GPU placement: it passes every check that looks at the tensor alone, so the
    checks behind the first operand are reached without a device"""

    class Fake(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)

    return torch.zeros(shape, dtype=torch.float64, device="meta").as_subclass(Fake)


def test_python_side_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    from genfer_amd import series2
    from genfer_amd.taylor import TaylorError

    x = torch.ones((3, 4, 8), dtype=torch.float64)
    # var is judged before anything else
    for bad in (2, -1, 1.0, "0", None, True):
        with pytest.raises(TaylorError, match="is 0 or 1"):
            series2.compose(x, x, var=bad)
    # and so is the exponent
    with pytest.raises(TaylorError, match="negative"):
        series2.pow(x, -1)
    for bad in (2.5, 2.0, "3", None, True):
        with pytest.raises(TypeError, match="non-negative integer"):
            series2.pow(x, bad)
    with pytest.raises(TaylorError, match="32 bits"):
        series2.pow(x, 2**32)
    for call in (lambda *a, **k: series2.compose(a[0], a[0], *a[1:], **k), lambda *a, **k: series2.compose(a[0], a[0], 1, *a[1:], **k),
                 lambda *a, **k: series2.pow(a[0], 3, *a[1:], **k)):
        with pytest.raises(TaylorError, match="float32"):
            call(x.float())
        with pytest.raises(TaylorError, match="at least 2"):
            call(x[0, 0])
        with pytest.raises(TaylorError, match="unit stride"):
            call(x[:, :, ::2])
        with pytest.raises(TaylorError, match="nx > n"):  # a stored length above n, on either axis
            call(x, n=(4, 7))
        with pytest.raises(TaylorError, match="nx > n"):
            call(x, n=(3, 8))
        with pytest.raises(TaylorError, match="n == 0"):
            call(x, n=(0, 8))
        with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
            call(x, n=(17, 241))  # 4097
        with pytest.raises(TaylorError, match=r"out has \(4, 9\)"):
            call(x, out=torch.empty((3, 4, 9), dtype=torch.float64))
        with pytest.raises(TaylorError, match="no autograd"):
            call(x.clone().requires_grad_())
        with pytest.raises(TaylorError, match="on cpu"):  # everything else in order: the placement is judged last
            call(x)
        with pytest.raises(TypeError, match="torch.Tensor"):
            call([[1.0, 2.0]])
    with pytest.raises(TaylorError, match="nx > n"):
        series2.compose(x[:, :2], x, n=(2, 8))  # g is the long one
    with pytest.raises(TaylorError, match="no autograd"):
        series2.compose(x, x.clone().requires_grad_())
    with pytest.raises(TaylorError, match="f: .*on cpu"):
        series2.compose(x, x)
    # behind a first operand that reports a GPU: the second operand's placement, by name
    f = _device_like(torch, (3, 4, 8))
    with pytest.raises(TaylorError, match="g: .*on cpu"):
        series2.compose(f, x)
    with pytest.raises(TaylorError, match="nx > n"):
        series2.compose(f, _device_like(torch, (3, 5, 8)), n=(4, 8))
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series2.pow(f, 2, n=(64, 65))


def test_bench_series2_knows_the_new_operations():
    spec = importlib.util.spec_from_file_location("bench_series2", os.path.join(ROOT, "tools", "bench_series2.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse_args(["--ops", "compose,pow"])
    assert args.ops == "compose,pow"
    with pytest.raises(SystemExit):
        mod.parse_args(["--ops", "compose,sqrt"])


# ---- the definition ----------------------------------------------------------------------------------------------------------------


def test_chain_equals_the_oracle(OTP, oracle_lib):
    """on dense and mixed-sign data the oracle's subst_var takes its general Horner path and pow its square-and-multiply, every
    product the general one: the chains the GPU tests use as expected values are the same functions, bit for bit"""
    seen = {"compose": 0, "pow": 0}
    for n in cc.ORACLE_SHAPES:
        for var, fs, gs, kind in cc.oracle_compose_cases(n):
            f, g = cc.make(kind, fs, 100 * n[0] + n[1] + var), cc.make(kind, gs, 100 * n[0] + n[1] + 7)
            ok = bits_equal(cc.chain_compose(oracle_lib, f, g, var, n), cc.oracle_compose(OTP, f, g, var, n))
            assert ok.all(), ("compose", n, var, fs, gs, kind)
            seen["compose"] += 1
        for xs, kind, e in cc.oracle_pow_cases(n):
            x = cc.make(kind, xs, 31 * n[0] + n[1])
            ok = bits_equal(cc.chain_pow(oracle_lib, x, e, n), cc.oracle_pow(OTP, x, e, n))
            assert ok.all(), ("pow", n, xs, kind, e)
            seen["pow"] += 1
    assert seen["compose"] + seen["pow"] >= 300 and seen["compose"] >= 150 and seen["pow"] >= 100, seen


INF, NAN = float("inf"), float("nan")


def test_chain_is_the_written_definition(oracle_lib):
    """the chain against the loops written out in numpy scalars, where the oracle's operators would shortcut: infinities, NaNs and
    zeros of both signs, g of stored shape (1, 1), one-slice f"""
    n = (4, 5)
    plain = dense(n, 71)
    fs = []
    for (i, j, v) in [(1, 1, INF), (0, 2, -INF), (2, 0, NAN), (3, 4, INF)]:
        a = plain.copy()
        a[i, j] = v
        fs.append(a)
    z = plain.copy()
    z[1:, :] = 0.0
    z[0, 2:] = -0.0
    fs += [z, -z, np.where(np.eye(*n) > 0, 1.0, np.where(plain > 1.0, -0.0, 0.0)), np.zeros(n), -np.zeros(n)]
    gs = [dense((3, 3), 72), np.array([[0.0, 1.0], [-0.0, INF]]), np.array([[0.75]]), np.array([[-0.0]]), np.array([[0.0, 1.0, 0.0]]),
          np.array([[0.0], [1.0]]), np.array([[NAN, 0.5], [1.0, 0.0]]), plain[::-1].copy()]
    checked = 0
    for var in (0, 1):
        for f in fs:
            for g in gs:
                ok = bits_equal(cc.chain_compose(oracle_lib, f, g, var, n), cc.model_compose(f, g, var, n))
                assert ok.all(), ("compose", var, f, g)
                checked += 1
        for g in gs:  # one slice of f: 0.0 + f padded, whatever g holds
            f = -z[:1] if var == 0 else -z[:, :1]
            got = cc.chain_compose(oracle_lib, f, g, var, n)
            assert bits_equal(got, cc.model_compose(f, g, var, n)).all()
            assert bits_equal(got, cc.pad2(0.0 + f, n)).all() and not (np.signbit(got) & (got == 0.0)).any()  # no -0.0 survives
    for x in fs + [np.array([[0.75]]), np.array([[-0.0]]), np.array([[-0.0, 2.0]]), np.array([[INF], [-0.0]])]:
        for e in (0, 1, 2, 3, 5):
            assert bits_equal(cc.chain_pow(oracle_lib, x, e, n), cc.model_pow(x, e, n)).all(), ("pow", x, e)
            checked += 1
    assert checked >= 200


# ---- the gfx950 code ---------------------------------------------------------------------------------------------------------------


def test_series2_compose_isa(tmp_path):
    """The gfx950 code of k_series2_compose<true> and <false> (tests/series2_compose_isa_check.hip): no private segment, no calls,
    LDS reads, separately rounded v_mul_f64 / v_add_f64 and no fused multiply-add of any spelling, no division or reciprocal in
    f64, and the barrier between the steps."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", "series2_compose_isa_check.hip")],
                          cwd=tmp_path)
    isa = open(glob.glob(str(tmp_path / "*amdgcn-amd-amdhsa*gfx950*.s"))[0]).read()
    kernels = {}
    private = {}
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
    for m in re.finditer(r"\.name:\s+(_ZN3gft\w+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", isa):
        private[m.group(1)] = int(m.group(2))
    both = {glds: [k for k in kernels if f"k_series2_composeILb{glds}E" in k] for glds in (0, 1)}
    assert all(len(v) == 1 for v in both.values()), list(kernels)
    for glds, (k,) in both.items():
        code = kernels[k]
        assert len(code) > 50
        assert private[k] == 0, (k, private)
        assert not [c for c in code if c.startswith("scratch_") or c.startswith("buffer_")]
        assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")]
        assert any(c.startswith("ds_read") or c.startswith("ds_load") for c in code)
        assert any(c.startswith("v_mul_f64") for c in code) and any(c.startswith("v_add_f64") for c in code)
        assert not [c for c in code if "fma" in c or c.startswith("v_fmac") or c.startswith("v_mad_f64")], "a contracted multiply-add"
        assert not [c for c in code if c.startswith("v_div_") or c.startswith("v_rcp_f64")]
        assert any(c == "s_barrier" for c in code)
