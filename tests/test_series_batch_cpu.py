"""Batched series (genfer_amd.series, gft_series_*) without a GPU: the exported and declared surface, the refusals the Python
side makes before it touches the library, the measurement tool's command line, and the gfx950 code of the form-A kernels."""
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

SYMBOLS = ("gft_series_mul", "gft_series_div", "gft_series_exp", "gft_series_log")


def test_symbols_are_declared_and_exported():
    import genfer_amd

    if not os.path.exists(genfer_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    L = genfer_amd.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS + ("gft_series_last_form",):
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert hasattr(L, s), s
        assert f"pub fn {s}(" in doc, s
    from genfer_amd.taylor import HANDLE_API

    assert not [n for n in HANDLE_API if n.startswith("series")]  # raw entry points: no gfti_ twin
    assert L.gft_set_option(b"series_form", 0.0) == 0


def test_module_is_re_exported():
    import genfer_amd
    from genfer_amd import series

    assert genfer_amd.series is series
    for f in ("mul", "div", "exp", "log"):
        assert callable(getattr(series, f))


def test_python_side_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    x = torch.zeros((3, 8), dtype=torch.float64)
    for f in (series.mul, series.div):
        with pytest.raises(TaylorError, match="on cpu"):
            f(x, x)
        with pytest.raises(TaylorError, match="float32"):
            f(x.float(), x)
    for f in (series.exp, series.log):
        with pytest.raises(TaylorError, match="on cpu"):
            f(x)
        with pytest.raises(TaylorError, match="float32"):
            f(x.float())
    with pytest.raises(TypeError, match="torch.Tensor"):
        series.mul([1.0, 2.0], x)
    # the order of the checks that need no device, on tensors of the meta device standing in for device tensors
    m = torch.zeros((3, 8), dtype=torch.float64, device="meta")
    with pytest.raises(TaylorError, match="on meta"):
        series.mul(m, m)


def test_order_checks():
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    assert series._order("t", None, 5, 9) == 9 and series._order("t", 12, 5, 9) == 12 and series._order("t", 4096, 1) == 4096
    with pytest.raises(TaylorError, match="4096"):
        series._order("t", 4097, 8)
    with pytest.raises(TaylorError, match="nx > n"):
        series._order("t", 4, 8)
    with pytest.raises(TaylorError, match="n == 0"):
        series._order("t", 0, 0)


def test_bench_series_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_series.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "--form" in out.stdout and "--ops" in out.stdout


def test_series_isa(tmp_path):
    """The gfx950 code of the form-A mul and div kernels (tests/series_isa_check.hip): no scratch, no buffer instructions, no
    calls, and no contracted multiply-add — the mul kernel has no FMA at all, the div kernel's are the five of its one IEEE
    f64 division sequence (v_div_fmas_f64)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", "series_isa_check.hip")],
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
    mul = [c for k, c in kernels.items() if "k_series_mul_a" in k]
    div = [c for k, c in kernels.items() if "k_series_div_a" in k]
    assert len(mul) == 1 and len(div) == 1 and len(mul[0]) > 50 and len(div[0]) > 50
    is_fma = lambda c: c in ("v_fma_f64", "v_fmac_f64_e32", "v_fmac_f64_e64", "v_pk_fma_f64")  # noqa: E731
    for code in (mul[0], div[0]):
        assert not [c for c in code if c.startswith("scratch_") or c.startswith("buffer_")]
        assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")]
        assert any(c.startswith("ds_read") or c.startswith("ds_load") for c in code)
        assert any(c == "v_mul_f64" or c.startswith("v_mul_f64") for c in code) and any(c.startswith("v_add_f64") for c in code)
    assert sum(map(is_fma, mul[0])) == 0 and mul[0].count("v_div_fmas_f64") == 0
    assert div[0].count("v_div_fmas_f64") >= 1 and sum(map(is_fma, div[0])) == 5 * div[0].count("v_div_fmas_f64")
