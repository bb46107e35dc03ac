"""BigFloat planes (src/number/big_float.rs): a value is {factor, exponent} with the factor in +-[1, 2), or 0, or
non-finite, meaning factor * 2**exponent.  On the C ABI a BigFloat tensor is plane-major like an interval tensor: the
factor plane, then the exponent plane (integral doubles).  These helpers convert float arrays to and from that form."""
import numpy as np


def encode(x, exponent_offset=0):
    """(factors, exponents) of float array `x` as big_float.rs `normalize` makes them, every exponent raised by
    `exponent_offset`: zeros (either sign) give {+0, 0}, non-finite values keep exponent `exponent_offset`."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)  # x = m * 2**e, |m| in [0.5, 1): exact, subnormals included
    f = m * 2.0
    e = e.astype(np.float64) - 1.0 + exponent_offset
    fin = np.isfinite(x)
    f = np.where(fin, f, x)
    e = np.where(fin, e, float(exponent_offset))
    zero = x == 0.0
    return np.where(zero, 0.0, f), np.where(zero, 0.0, e)


def powi2(n):
    """f64::powi(2.0, n as i32) as the project lowers it: exactly 2**n for -1023 <= n <= 1023, +0 below, +inf above."""
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(over="ignore"):
        p = np.ldexp(1.0, np.clip(n, -1024, 1024).astype(np.int64))
    return np.where(n <= -1024, 0.0, np.where(n >= 1024, np.inf, p))


def decode(factors, exponents):
    """big_float.rs `to_f64`: factor * powi(2, exponent) (inf * 0 is NaN, as there)."""
    f = np.asarray(factors, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return f * powi2(exponents)
