"""The exponential of a truncated multivariate power series in exact rational arithmetic (fractions.Fraction), from the
definition: E = exp(f) is the series with E(0) = 1 and dE/dx0 = (df/dx0) E, i.e. along axis 0

    k E[k] = sum_{j = 1..k} j f[j] (*) E[k - j]          ((*): the truncated product over the remaining axes)

with E[0] = exp(f[0]) one rank lower, and exp of a rank-0 series with zero constant term equal to 1.  A non-zero
constant term c0 is a factor by linearity: exp(a) = exp(c0) exp(a - c0).  Nothing here touches the oracle or the library;
the reference of the right-looking exp tests (test_exp_right_cpu.py, test_exp_right_gpu.py)."""
from fractions import Fraction

import numpy as np


def to_fractions(a):
    """f64 array -> object array of the exact rationals the doubles are."""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for i in np.ndindex(a.shape):
        out[i] = Fraction(float(a[i]))
    return out


def frac_conv(x, y, zshape):
    """Truncated product of two object (Fraction) arrays of one rank into `zshape`: one shifted slice multiply-add per
    non-zero coefficient of x."""
    z = np.empty(zshape, dtype=object)
    z.fill(Fraction(0))
    for idx in np.ndindex(x.shape):
        c = x[idx]
        if c == 0:
            continue
        ext = tuple(min(zs - i, ys) for zs, i, ys in zip(zshape, idx, y.shape))
        if min(ext) <= 0:
            continue
        dst = tuple(slice(i, i + e) for i, e in zip(idx, ext))
        src = tuple(slice(0, e) for e in ext)
        z[dst] = z[dst] + c * y[src]
    return z


def exp_series(f, shape):
    """exp of the series with (compact) Fraction coefficients `f`, f[0, .., 0] == 0, truncated to `shape` (>= f.shape)."""
    assert f.ndim == len(shape) and all(a <= b for a, b in zip(f.shape, shape))
    if f.ndim == 0:
        assert f[()] == 0
        return np.asarray(Fraction(1), dtype=object)
    E = np.empty(shape, dtype=object)
    E.fill(Fraction(0))
    if f.ndim == 1:  # scalars: k E[k] = sum_j j f[j] E[k - j]
        assert f[0] == 0
        E[0] = Fraction(1)
        for k in range(1, shape[0]):
            E[k] = sum((j * f[j] * E[k - j] for j in range(1, min(k, f.shape[0] - 1) + 1)), Fraction(0)) / k
        return E
    rest = tuple(shape[1:])
    E[0] = exp_series(f[0], rest)
    for k in range(1, shape[0]):
        acc = np.empty(rest, dtype=object)
        acc.fill(Fraction(0))
        for j in range(1, min(k, f.shape[0] - 1) + 1):
            acc = acc + j * frac_conv(f[j], E[k - j], rest)
        E[k] = acc / Fraction(k)
    return E


def exp_exact(a, shape):
    """(c0, E, M) for an f64 argument `a` (compact) and result `shape`: the constant term, the exact exponential of
    a - c0 and its majorant, the exact exponential of |a - c0| — both without the factor exp(c0)."""
    f = to_fractions(a)
    c0 = f[(0,) * f.ndim]
    f[(0,) * f.ndim] = Fraction(0)
    E = exp_series(f, tuple(shape))
    absf = np.empty(f.shape, dtype=object)
    for i in np.ndindex(f.shape):
        absf[i] = abs(f[i])
    M = E if all(f[i] >= 0 for i in np.ndindex(f.shape)) else exp_series(absf, tuple(shape))
    return float(c0), E, M


def worst_ratio(got, E, M, seed):
    """max over the coefficients of |got - seed E| / (seed M), exactly (a Fraction); `seed` = got[0, .., 0], the f64 value
    of exp(c0) the recurrence started from.  Coefficients with M == 0 must be exact zeros (ratio infinite otherwise)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == E.shape, (got.shape, E.shape)
    s = Fraction(float(seed))
    worst = Fraction(0)
    for i in np.ndindex(E.shape):
        g = float(got[i])
        if g != g or g in (float("inf"), float("-inf")):
            return Fraction(10) ** 300
        err = abs(Fraction(g) - s * E[i])
        if M[i] == 0:
            if err != 0:
                return Fraction(10) ** 300
            continue
        worst = max(worst, err / (s * M[i]))
    return worst


# ---- the cases of the right-looking exp tests (shared by the CPU twin and the GPU file) ---------------------------------
# name: (degree caps, stored operand shape, tiled products expected).  The result's shape is the caps, with 1 on every axis
# on which the operand has 1 (explog_shape).  `tiled` is the number of accumulate-mode products of the right-looking loop
# that reach the tiled kernel with tiled_min_macs lowered to 1: one per step with work (n - 1 for a full operand) on every
# recursion level of rank >= 3, plus — where the rank-2 base has fewer than 8 rows, so that its wavefront declines and the
# loop runs there too — its steps of two or more slabs (a one-slab step of rank 2 collapses to rank 1: reference order).
CASES = {
    "full_inner28": ((6, 5, 28), (6, 5, 28), 5 + 3),          # packed rows
    "full_inner8": ((5, 9, 8), (5, 9, 8), 4),                 # rows of one whole chunk
    "full_inner16": ((5, 6, 16), (5, 6, 16), 4 + 4),
    "full_inner32": ((3, 10, 32), (3, 10, 32), 2),
    "single_step": ((2, 9, 12), (2, 9, 12), 1),               # n0 = 2
    "lead2_under_6": ((6, 9, 12), (2, 9, 12), 5),             # m capped by the operand: min(n0 - 1 - i, 1)
    "lead3_under_6": ((6, 9, 12), (3, 9, 12), 5),
    "compact_mid_last": ((5, 9, 16), (5, 6, 11), 4),          # rows end inside a chunk
    "unit_lead": ((4, 9, 12), (1, 9, 12), 0),                 # a unit operand axis is a unit RESULT axis: rank 2, the wavefront
    "unit_middle": ((5, 9, 12), (5, 1, 12), 3),               # steps are (m, 12) products; the last (m = 1) is rank 1
    "unit_last": ((5, 9, 12), (5, 9, 1), 3),
    "rank4": ((3, 4, 9, 8), (3, 4, 9, 8), 2 + 3),
    "rank5": ((3, 2, 3, 9, 8), (3, 2, 3, 9, 8), 1 + 1 + 2),   # the rank-5 step of two slabs: reference order (see the GPU test)
    "last_over_128": ((3, 3, 130), (3, 3, 130), 2 + 1),       # the inner split with accumulate, slab range and fold
}


def case_data(name, positive=False):
    """The dyadic argument of a case: k / 64 with |k| <= 16 (exact in f64, few bits), constant term 1/2 or -1/4."""
    import zlib

    deg, xs, _ = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) + (1 if positive else 0))
    a = rng.integers(0 if positive else -16, 17, size=xs).astype(np.float64) / 64.0
    a[(0,) * len(xs)] = -0.25 if positive else 0.5
    return a


def result_shape(deg, xs):
    return tuple(1 if x == 1 else d for d, x in zip(deg, xs))


_REFERENCES = {}


def case_reference(name, positive=False):
    """(a, c0, E, M) of a case, computed once per process."""
    key = (name, positive)
    if key not in _REFERENCES:
        deg, xs, _ = CASES[name]
        a = case_data(name, positive)
        _REFERENCES[key] = (a,) + exp_exact(a, result_shape(deg, xs))
    return _REFERENCES[key]
