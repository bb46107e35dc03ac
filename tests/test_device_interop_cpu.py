"""Device interop without a GPU: the C surface of gft_from_device / gft_to_device (declared, exported, in the Rust extern
block), and the Python layer's refusals that happen before any call into the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

INTEROP = ("gft_from_device", "gft_to_device", "gfti_from_device", "gfti_to_device", "gft_device")


@pytest.fixture(scope="module")
def product_lib():
    import genfer_amd

    if not os.path.exists(genfer_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return genfer_amd.lib()


def test_header_declares_device_interop():
    text = open(os.path.join(ROOT, "include", "gftaylor.h")).read()
    assert "gft_poly* gft_from_device(const double* src, const int64_t* strides, const size_t* shape" in text
    assert "int gft_to_device(const gft_poly* p, double* dst, const int64_t* strides, void* stream);" in text
    assert "gft_poly* gfti_from_device(const double* src, const int64_t* strides" in text
    assert "int gfti_to_device(const gft_poly* p, double* dst, const int64_t* strides, void* stream);" in text
    assert "int gft_device(void);" in text


def test_library_exports_device_interop(product_lib):
    for name in INTEROP:
        assert hasattr(product_lib, name), name


def test_rust_extern_block_is_current():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_extern.py"), "--check"])
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub fn gft_from_device(src: *const f64, strides: *const i64," in doc
    assert "pub fn gfti_to_device(p: *const GftPoly, dst: *mut f64, strides: *const i64, stream: *mut c_void) -> c_int;" in doc


def test_device_api_not_in_handle_table():
    from genfer_amd.taylor import DEVICE_API, HANDLE_API

    assert not set(DEVICE_API) & set(HANDLE_API)


@pytest.mark.parametrize("cls", ["OTP", "OTPI"])
def test_oracle_classes_have_no_device_interop(cls, request):
    from genfer_amd.taylor import TaylorError

    TP = request.getfixturevalue(cls)
    assert not TP._fn.device_interop
    with pytest.raises(TaylorError, match="no device interop"):
        TP.from_torch(None)
    p = TP.from_coeffs(np.ones((2, 3)) if TP.WIDTH == 1 else np.ones((2, 2, 3)))
    with pytest.raises(TaylorError, match="no device interop"):
        p.to_torch()


class _Trap:
    """Stands in for a bound entry point: any call fails the test."""

    def __init__(self, name):
        self.name = name

    def __call__(self, *a):
        raise AssertionError(f"{self.name} was called")


@pytest.mark.parametrize("prefix", ["gft_", "gfti_"])
def test_cpu_and_float32_tensors_refused_before_any_c_call(prefix, product_lib):
    torch = pytest.importorskip("torch")
    import genfer_amd
    from genfer_amd.taylor import TaylorError

    TP = genfer_amd.TaylorPoly if prefix == "gft_" else genfer_amd.IntervalTaylorPoly
    fn = TP._fn
    saved = {n: getattr(fn, n) for n in ("from_device", "to_device", "device")}
    try:
        for n in saved:
            setattr(fn, n, _Trap(n))
        shape = (3, 4) if prefix == "gft_" else (2, 3, 4)
        with pytest.raises(TaylorError, match="float32"):
            TP.from_torch(torch.zeros(shape, dtype=torch.float32))
        with pytest.raises(TaylorError, match="on cpu"):
            TP.from_torch(torch.zeros(shape, dtype=torch.float64))
        with pytest.raises(TypeError):
            TP.from_torch(np.zeros(shape))
    finally:
        for n, f in saved.items():
            setattr(fn, n, f)
