"""Batched bivariate series (genfer_amd.series2, gft_series2_*) without a GPU: the plain-Python model of the four recursions
against the CPU oracle, the exported and declared surface, the refusals the Python side makes before it touches a device, the
measurement tool's command line, and the gfx950 code of the kernels."""
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _series2_model as model
from _series2_oracle import OPS, bits_equal, compact_shapes, dense, oracle_is_normative, signed, want
from conftest import ROOT

SHAPES = [(2, 2), (3, 5), (5, 3), (8, 8), (1, 6), (6, 1), (4, 17), (12, 7)]
KINDS = ("dense", "compact", "signed")
SYMBOLS = ("gft_series2_mul", "gft_series2_div", "gft_series2_exp", "gft_series2_log")


def operands(kind, n, seed):
    xs, ys = compact_shapes(*n) if kind == "compact" else (n, n)
    make = signed if kind == "signed" else dense
    return make(xs, seed), make(ys, seed + 1)


def model_item(op, x, y, n):
    return getattr(model, op)(x, y, n) if op in ("mul", "div") else getattr(model, op)(x, n)


@pytest.mark.parametrize("op", OPS)
def test_model_against_the_oracle(op, OTP, oracle_lib):
    """bit for bit wherever the oracle is normative (the divisor / the operand of log keeps 2 coefficients on both axes); value
    for value (==: signs of zeros may differ) on the remaining cases, where the reference shortcuts or stores fewer rows"""
    exact = valued = 0
    for n in SHAPES:
        for kind in KINDS:
            x, y = operands(kind, n, 100 * n[0] + n[1])
            got = model_item(op, x, y, n)
            exp = want(oracle_lib, OTP, op, x[None], y[None], n)[0]
            what = f"{op} n={n} {kind}"
            if oracle_is_normative(op, x, y):
                ok = bits_equal(got, exp)
                assert ok.all(), (what, got[~ok], exp[~ok])
                exact += 1
            else:
                assert np.array_equal(got, exp), (what, got, exp)
                valued += 1
    assert exact + valued == len(SHAPES) * len(KINDS) and exact >= 16
    assert (valued > 0) == (op in ("div", "log"))


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


def test_module_is_re_exported():
    import genfer_amd
    from genfer_amd import series2

    assert genfer_amd.series2 is series2
    for f in OPS:
        assert callable(getattr(series2, f))
    assert series2.MAX_ELEMS == 4096


def test_python_side_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    from genfer_amd import series2
    from genfer_amd.taylor import TaylorError

    x = torch.ones((3, 4, 8), dtype=torch.float64)
    binary, unary = (series2.mul, series2.div), (series2.exp, series2.log)
    for f in binary + unary:
        call = (lambda *a, **k: f(a[0], a[0], *a[1:], **k)) if f in binary else f  # noqa: E731
        with pytest.raises(TaylorError, match="float32"):
            call(x.float())
        with pytest.raises(TaylorError, match="at least 2"):
            call(x[0, 0])
        with pytest.raises(TaylorError, match="is empty"):
            call(x[:, :0])
        with pytest.raises(TaylorError, match="is empty"):
            call(x[:, :, :0])
        with pytest.raises(TaylorError, match="unit stride"):
            call(x[:, :, ::2])
        with pytest.raises(TaylorError, match="nx > n"):
            call(x, n=(4, 7))
        with pytest.raises(TaylorError, match="nx > n"):
            call(x, n=(3, 8))
        with pytest.raises(TaylorError, match="n == 0"):
            call(x, n=(0, 8))
        with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
            call(x, n=(17, 241))  # 4097
        with pytest.raises(TaylorError, match=r"out has \(4, 9\)"):
            call(x, out=torch.empty((3, 4, 9), dtype=torch.float64))
        with pytest.raises(TaylorError, match="batch shape"):
            call(x, out=torch.empty((1, 4, 8), dtype=torch.float64))
        with pytest.raises(TaylorError, match="no autograd"):
            call(x.clone().requires_grad_())
        with pytest.raises(TaylorError, match="on cpu"):  # everything else in order: the placement is judged last
            call(x)
        with pytest.raises(TypeError, match="torch.Tensor"):
            call([[1.0, 2.0]])
        with pytest.raises(TypeError, match="pair"):
            call(x, n=8)
    with torch.no_grad():  # grad mode off: the operand is taken as it is (and then refused for where it lives)
        with pytest.raises(TaylorError, match="on cpu"):
            series2.exp(x.clone().requires_grad_())
    with pytest.raises(TaylorError, match="nx > n"):
        series2.mul(x[:, :2], x, n=(2, 8))  # y is the long one
    m = torch.zeros((3, 4, 8), dtype=torch.float64, device="meta")
    with pytest.raises(TaylorError, match="on meta"):
        series2.mul(m, m)


def test_bench_series2_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_series2.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "--shapes" in out.stdout and "--ops" in out.stdout


def test_series2_isa(tmp_path):
    """The gfx950 code of the four kernels (tests/series2_isa_check.hip): no scratch, no buffer instructions, no calls; the mul
    kernel has no FMA at all, the div kernel's are the five of each IEEE f64 division sequence (v_div_fmas_f64)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", "series2_isa_check.hip")],
                          cwd=tmp_path)
    isa = open(glob.glob(str(tmp_path / "*amdgcn-amd-amdhsa*gfx950*.s"))[0]).read()
    assert isa.count(".private_segment_fixed_size: 0") == 4 and isa.count(".private_segment_fixed_size:") == 4
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
    mul = [c for k, c in kernels.items() if "k_series2_mul" in k]
    rec = {op: [c for k, c in kernels.items() if f"k_series2_recILi{op}E" in k] for op in (1, 2, 3)}  # SERIES_DIV, _EXP, _LOG
    assert len(mul) == 1 and all(len(v) == 1 for v in rec.values())
    is_fma = lambda c: c in ("v_fma_f64", "v_fmac_f64_e32", "v_fmac_f64_e64", "v_pk_fma_f64")  # noqa: E731
    for code in (mul[0], rec[1][0], rec[2][0], rec[3][0]):
        assert len(code) > 50
        assert not [c for c in code if c.startswith("scratch_") or c.startswith("buffer_")]
        assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")]
        assert any(c.startswith("ds_read") or c.startswith("ds_load") for c in code)
        assert any(c.startswith("v_mul_f64") for c in code) and any(c.startswith("v_add_f64") for c in code)
    assert sum(map(is_fma, mul[0])) == 0 and mul[0].count("v_div_fmas_f64") == 0
    div = rec[1][0]
    assert div.count("v_div_fmas_f64") >= 1 and sum(map(is_fma, div)) == 5 * div.count("v_div_fmas_f64")
