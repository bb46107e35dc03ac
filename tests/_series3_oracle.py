"""Expected values and operands shared by tests/test_series3_cpu.py and tests/test_series3_gpu.py: the CPU oracle at rank 3, one item
at a time, and the two kinds of data (dense, mixed signs)."""
import ctypes as C
import math

import numpy as np

import _series3_model as model
from _series2_oracle import assert_bits, bits_equal  # noqa: F401  (re-exported)
from conftest import splitmix64_uniform

OPS = ("mul", "div", "exp", "log")


def dense(shape, seed):
    """0.5 + uniform: no operand is zero, one, constant or linear -- the oracle's operators take no data-dependent shortcut"""
    return (0.5 + splitmix64_uniform(seed, int(np.prod(shape)))).reshape(shape)


def signed(shape, seed):
    """uniform in [-0.5, 0.5) with coefficient [..., 0, 0, 0] in [1.0, 1.5): a divisor away from zero, a positive operand of log"""
    a = (splitmix64_uniform(seed, int(np.prod(shape))) - 0.5).reshape(shape)
    a[..., 0, 0, 0] = np.abs(a[..., 0, 0, 0]) + 1.0
    return a


def pad3(a, n):
    out = np.zeros(n)
    a = np.asarray(a, dtype=np.float64)
    out[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    return out


def want(oracle_lib, OTP, op, x, y, n):
    """x: [B, nx0, nx1, nx2].  mul: orc_mul_raw at rank 3 on a zeroed result of the stored shape S (the general product, no
    dispatcher); div / exp / log: the oracle's operators (platform libm seeds).  What the oracle leaves unstored is +0."""
    n = tuple(n)
    out = np.zeros((x.shape[0],) + n)
    if op == "mul":
        szp = C.POINTER(C.c_size_t)
        oracle_lib.orc_mul_raw.restype = C.c_int
        oracle_lib.orc_mul_raw.argtypes = [C.c_void_p, szp, C.c_void_p, szp, C.c_void_p, szp, C.c_size_t]
        three = lambda s: (C.c_size_t * 3)(*s)  # noqa: E731
        s = model.result_shape("mul", n, x.shape[1:], y.shape[1:])
    for b in range(x.shape[0]):
        if op == "mul":
            xr, yr, z = np.ascontiguousarray(x[b]), np.ascontiguousarray(y[b]), np.zeros(s)
            assert oracle_lib.orc_mul_raw(xr.ctypes.data_as(C.c_void_p), three(xr.shape), yr.ctypes.data_as(C.c_void_p), three(yr.shape),
                                          z.ctypes.data_as(C.c_void_p), three(s), 3) == 0
            out[b] = pad3(z, n)
        else:
            p = OTP.new(x[b], n)
            r = p / OTP.new(y[b], n) if op == "div" else (p.exp() if op == "exp" else p.log())
            out[b] = pad3(r.array(), n)
    return out


def host_seeds(op, x):
    f = math.exp if op == "exp" else math.log
    return np.array([f(v) for v in x.reshape(x.shape[0], -1)[:, 0]])


def oracle_is_normative(op, x, y):
    """the oracle's operators take one shape-triggered shortcut: a divisor of one stored coefficient.  There the loops are the
    definition (tests/_series3_model.py)."""
    return op != "div" or int(np.prod(y.shape[-3:])) > 1


def model_batch(op, x, y, n, seeds=None):
    f = getattr(model, op)
    if op in ("mul", "div"):
        return np.stack([f(x[b], y[b], n) for b in range(x.shape[0])])
    return np.stack([f(x[b], n, None if seeds is None else seeds[b]) for b in range(x.shape[0])])
