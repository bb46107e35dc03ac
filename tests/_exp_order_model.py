"""Cases, data and the ordered model of exp in arrival order, for test_exp_arrival_order_cpu.py and test_exp_arrival_order_gpu.py.

`exp` of a rank-2 f64 series has two summation orders on the device.  Where Ops<E>::exp_rec (gft_ops_recur.inc) would
take the right-looking tiled form (f64, `conv_mode` 0, `exp_right`, prod_i (0.5 n_i min(xn_i, n_i) + 0.5) >=
64 `tiled_min_macs`) it runs the one-launch wavefront with `rev` = 1: every row's source rows in DESCENDING j0, the order
in which they become available (gft_div2d.hip, the comment above k_rows_wavefront; `rev` in gft_wavefront_plan.hpp).
Everywhere else the source rows come in the reference's ascending order.

The model (exp_order_model.cpp, compiled on first use with -ffp-contract=off like the library) performs the same IEEE
operations in either order; it shares no code with the oracle or the kernels.  Ascending it must be the oracle's bits,
descending the bits of the `rev` kernels.
"""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np

from conftest import load_oracle_lib, splitmix64_uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILED_MIN_MACS_DEFAULT = 2e5  # R.tiled_min_macs (gft_api.hip)
# WF_NW_F64 (gft_wavefront_plan.hpp) = DwfCfg<EF64>::NW (gft_div2d.hip): source rows per batch of the unpacked k_div_wavefront and
# of k_rows_wavefront.  A literal, so that the case ids need no compiler at collection; batch_rows() is the header's value.
NW = 16


def rand(shape, seed, lo=0.0, hi=1.0):
    n = int(np.prod(shape)) if len(shape) else 1
    return (lo + (hi - lo) * splitmix64_uniform(seed, n)).reshape(shape)


@functools.lru_cache(maxsize=None)
def _model_lib():
    d = tempfile.mkdtemp(prefix="exp_order_model_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libexp_order_model.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "genfer_amd", "csrc"), os.path.join(ROOT, "tests", "exp_order_model.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.exp_order_model.argtypes = [dp, ctypes.c_uint, ctypes.c_uint, dp, ctypes.c_uint, ctypes.c_uint, ctypes.c_int, dp]
    lib.exp_order_model.restype = ctypes.c_int
    lib.exp_plan_family.argtypes = [ctypes.c_uint] * 4 + [ctypes.c_int]
    lib.exp_plan_family.restype = ctypes.c_int
    lib.exp_batch_rows.argtypes = []
    lib.exp_batch_rows.restype = ctypes.c_uint
    return lib


PLAN_FAMILIES = ("none", "row", "quad16", "quad8", "rows2d", "seg")  # WfFamily (gft_wavefront_plan.hpp)


def planned(n, xn, arrival_order=True):
    """(family, rev) of plan_wavefront for exp at these extents."""
    v = _model_lib().exp_plan_family(n[0], n[1], xn[0], xn[1], int(arrival_order))
    return PLAN_FAMILIES[v % 16], v // 16


def batch_rows():
    return int(_model_lib().exp_batch_rows())


def exp_model(x, n, row0, descending):
    """res[n0, nr] = exp(x[xn0, xnr]) with the given row 0, every row's source rows in ascending or descending j0."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    row0 = np.ascontiguousarray(row0, dtype=np.float64)
    n0, nr = n
    assert x.ndim == 2 and row0.shape == (nr,) and x.shape[0] <= n0 and x.shape[1] <= nr
    res = np.empty((n0, nr), dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = _model_lib().exp_order_model(x.ctypes.data_as(dp), x.shape[0], x.shape[1], row0.ctypes.data_as(dp), n0, nr, int(bool(descending)),
                                      res.ctypes.data_as(dp))
    assert rc == 0
    return res


@functools.lru_cache(maxsize=None)
def OTP():
    """Oracle-backed TaylorPoly<F64> (the session fixture's class, for the module-level cache below)."""
    from genfer_amd.taylor import bind

    return bind(load_oracle_lib(), "orc_")


# ---- cases ------------------------------------------------------------------------------------------------------------------
# family: what plan_wavefront (gft_wavefront_plan.hpp) selects for the shape, or
#   "loop": no wavefront — the host-driven right-looking loop (contract check only)
#   "line": the argument has one coefficient per row, so the RESULT has one too (mt:406-417: an axis of extent 1 in the
#           argument has extent 1 in the result) — a 1-d exp whatever the degrees say; no wavefront, the reference's order
# special: None, or "inf" (x[2, 1] = inf), "nan" (x[1, 0] = nan), "wide" (x[0, 0] = 235: row 0 holds values >= 1e100)
def _case(n, xn=None, family="row", special=None):
    xn = n if xn is None else xn
    cid = f"{n[0]}x{n[1]}-arg{xn[0]}x{xn[1]}" + (f"-{special}" if special else "")
    return SimpleNamespace(id=cid, n=tuple(n), xn=tuple(xn), family=family, special=special)


K_BATCH = 2  # the batch-boundary rows: NW k - 1, NW k, NW k + 1 result rows
CASES = [
    _case((8, 2)),                                     # WF_ROW packed: the smallest shape the planner accepts (rows >= 8, nr >= 2)
    _case((21, 31)),                                   # WF_ROW packed: odd source counts, the upper half-wave's "next row" runs past the end
    _case((12, 32), (5, 32)),                          # WF_ROW packed: rows of exactly 32; compact xn0, cnt = min(k0, 4)
    _case((12, 32), (12, 1), family="line"),           # argument rows of one coefficient: the result is a line (see "line" above)
    _case((12, 32), (12, 2)),                          # WF_ROW packed: the thinnest argument rows that keep the result's rows
    _case((40, 33), (17, 20)),                         # WF_ROW unpacked: first unpacked length; compact on both axes
    # WF_ROW unpacked, rows of exactly 64, around a whole number of batches of NW source rows (row k0 has k0 sources, so the
    # last row has n0 - 1)
    _case((NW * K_BATCH - 1, 64)),
    _case((NW * K_BATCH, 64)),                         # the last row ends one short of a whole batch, ...
    _case((NW * K_BATCH + 1, 64)),                     # ... fills its last batch exactly, ...
    _case((NW * K_BATCH + 2, 64)),                     # ... and runs one source row into the next batch
    _case((2050, 9), family="quad8"),                  # WF_ROW_QUAD8: rows >= 2048; a long chain
    _case((2049, 33), (2049, 5), family="quad16"),     # WF_ROW_QUAD16: 16-lane groups; thin argument rows keep the model cheap
    _case((2047, 33), (2047, 5)),                      # WF_ROW: the row count just below the quad threshold, same data family
    _case((8, 65), family="rows2d"),                   # WF_ROWS_2D: one coefficient into segment 1
    _case((24, 130), family="rows2d"),                 # three segments, the last one partial
    _case((60, 200), (45, 150), family="rows2d"),      # compact argument whose rows end inside segment 2
    _case((9, 4096), (9, 70), family="rows2d"),        # the longest row the planner takes
    _case((9, 4097), (9, 70), family="loop"),          # wf_2d false: the host-driven loop just past the limit
    _case((6, 130), family="loop"),                    # rows < 8: the rank-2 right-looking loop with tiled products at a lowered threshold
    _case((24, 130), family="rows2d", special="inf"),
    _case((24, 130), family="rows2d", special="nan"),
    _case((24, 130), family="rows2d", special="wide"),
    _case((21, 31), special="inf"),
    _case((21, 31), special="nan"),
    _case((21, 31), special="wide"),
]
# the dispatch criterion itself, no option touched: (0.5 84^2 + 0.5)^2 = 1.245e7 < 64 * 2e5 = 1.28e7 <= 1.305e7 = (0.5 85^2 + 0.5)^2
SWITCH_BELOW = _case((84, 84), family="rows2d")
SWITCH_ABOVE = _case((85, 85), family="rows2d")
ALL_CASES = CASES + [SWITCH_BELOW, SWITCH_ABOVE]
BY_ID = {c.id: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES)

WAVEFRONT_FAMILIES = ("row", "quad8", "quad16", "rows2d")


def criterion(case):
    """exp_rec's `total` (gft_ops_recur.inc): the right-looking / arrival-order form is taken from 64 tiled_min_macs on."""
    total = 1.0
    for n, xn in zip(case.n, case.xn):
        total *= 0.5 * n * min(xn, n) + 0.5
    return total


def argument(case):
    x = rand(case.xn, 84, -0.3, 0.3)  # mixed signs: what the existing exp cases use (test_div_row_wavefront_bit_exact)
    if case.special == "inf":
        x[2, 1] = np.inf
    elif case.special == "nan":
        x[1, 0] = np.nan
    elif case.special == "wide":
        x[0, 0] = 235.0  # exp(235) = 1.1e102
    return x


@functools.lru_cache(maxsize=None)
def case_data(cid):
    """Everything the tests compare against, computed once per case and never modified (the arrays are read-only)."""
    case = BY_ID[cid]
    x = argument(case)
    deg = list(case.n)
    o = OTP().new(x, deg).exp()
    want = o.array()
    assert want.ndim == 2
    with np.errstate(all="ignore"):
        asc = exp_model(x, want.shape, want[0], False)
        desc = exp_model(x, want.shape, want[0], True)
        if case.special in ("inf", "nan"):
            # no finite bound exists; the base case's (x differs in that one entry) scales the recorded deviation of the
            # coefficients that stay finite, and no assertion uses it
            bound = case_data(_case(case.n, case.xn).id).bound
        else:
            bound = OTP().new(np.abs(x), deg).exp().array()
    for a in (x, want, asc, desc, bound):
        a.setflags(write=False)
    return SimpleNamespace(case=case, x=x, deg=deg, want=want, degrees_p1=o.degrees_p1(), asc=asc, desc=desc, bound=bound)
