"""Expected values and operands shared by tests/test_series2_cpu.py and tests/test_series2_gpu.py: the CPU oracle at rank 2, one
item at a time, and the three kinds of operands (dense, compact, mixed signs)."""
import ctypes as C
import math

import numpy as np

from conftest import splitmix64_uniform

OPS = ("mul", "div", "exp", "log")


def dense(shape, seed):
    """0.5 + uniform: dense arrays, divisors neither constant nor one -- the oracle takes no shortcut"""
    return (0.5 + splitmix64_uniform(seed, int(np.prod(shape)))).reshape(shape)


def signed(shape, seed):
    """uniform in [-0.5, 0.5) with coefficient [..., 0, 0] in [1.0, 1.5): a divisor away from zero, a positive operand of log"""
    a = (splitmix64_uniform(seed, int(np.prod(shape))) - 0.5).reshape(shape)
    a[..., 0, 0] = np.abs(a[..., 0, 0]) + 1.0
    return a


def compact_shapes(n0, n1):
    """the stored shapes of the compact operands x and y under a result of (n0, n1)"""
    return (max(1, n0 // 2), max(1, n1 - 1)), (max(1, n0 - 1), max(1, min(n1, max(2, n1 // 2))))


def pad2(a, n):
    out = np.zeros(n)
    a = np.asarray(a, dtype=np.float64)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def want_mul(oracle_lib, x, y, n):
    """orc_mul_raw at rank 2 on a zeroed result: the general product, no dispatcher.  x: [B, nx0, nx1], y: [B, ny0, ny1]"""
    szp = C.POINTER(C.c_size_t)
    oracle_lib.orc_mul_raw.restype = C.c_int
    oracle_lib.orc_mul_raw.argtypes = [C.c_void_p, szp, C.c_void_p, szp, C.c_void_p, szp, C.c_size_t]
    out = np.zeros((x.shape[0],) + tuple(n))
    two = lambda s: (C.c_size_t * 2)(*s)  # noqa: E731
    for b in range(x.shape[0]):
        xr, yr = np.ascontiguousarray(x[b]), np.ascontiguousarray(y[b])
        rc = oracle_lib.orc_mul_raw(xr.ctypes.data_as(C.c_void_p), two(xr.shape), yr.ctypes.data_as(C.c_void_p), two(yr.shape),
                                    out[b].ctypes.data_as(C.c_void_p), two(n), 2)
        assert rc == 0
    return out


def want_handle(OTP, op, x, y, n):
    """div / exp / log through the oracle's handle API (platform libm seeds); what the oracle leaves unstored is +0"""
    out = np.zeros((x.shape[0],) + tuple(n))
    for b in range(x.shape[0]):
        p = OTP.new(x[b], n)
        r = p / OTP.new(y[b], n) if op == "div" else (p.exp() if op == "exp" else p.log())
        out[b] = pad2(r.array(), n)
    return out


def want(oracle_lib, OTP, op, x, y, n):
    return want_mul(oracle_lib, x, y, n) if op == "mul" else want_handle(OTP, op, x, y, n)


def host_seeds(op, x):
    f = math.exp if op == "exp" else math.log
    return np.array([f(v) for v in x[:, 0, 0]])


def oracle_is_normative(op, x, y):
    """the oracle supplies the bits wherever the divisor of div / the operand of log stores at least 2 coefficients on both axes"""
    t = y if op == "div" else x
    return op in ("mul", "exp") or (t.shape[-2] >= 2 and t.shape[-1] >= 2)


def bits_equal(got, want):
    """every bit of every coefficient; where the expected value is NaN, a NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.where(np.isnan(want), np.isnan(got), got.view(np.int64) == want.view(np.int64))


def assert_bits(got, want, what):
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    ok = bits_equal(got, want)
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {(~ok).sum()} coefficients differ, first at {i}: got {got[i]!r} want {want[i]!r}")
