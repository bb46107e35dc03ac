"""The four bivariate recursions of genfer_amd.series2 (include/gftaylor.h) in plain Python, one IEEE operation at a time.

An item is a numpy float64 array ``[n0, n1]``; the operands may be smaller (compact).  Every multiply, add and divide is one
numpy float64 scalar operation, so the order written here is the order of the roundings.  ``mul1d`` / ``div1d`` / ``exp1d`` /
``log1d`` are the univariate loops of ``gft_series_*`` (sums from 0.0; ``log1d`` of a one-coefficient row stores +0 above
coefficient 0, as ``gft_series_log`` does)."""
import math

import numpy as np

F = np.float64
ZERO = F(0.0)


def mul1d(xs, ys, n):
    zs = [ZERO] * n
    for k in range(n):
        s = ZERO
        for j in range(max(0, k + 1 - len(ys)), min(k + 1, len(xs))):
            s = s + xs[j] * ys[k - j]
        zs[k] = s
    return zs


def div1d(xs, ys, n):
    """r[k] = (-(0 + sum_{j = lo .. k-1} r[j] * y[k-j]) + x[k]) / y[0]"""
    r = [ZERO] * n
    for k in range(n):
        s = ZERO
        for j in range(max(0, k + 1 - len(ys)), k):
            s = s + r[j] * ys[k - j]
        c = -s
        if k < len(xs):
            c = c + xs[k]
        r[k] = c / ys[0]
    return r


def exp1d(xs, n, seed):
    r = [ZERO] * n
    r[0] = F(seed)
    for k in range(1, n):
        s = ZERO
        for j in range(1, min(len(xs), k + 1)):
            s = s + (xs[j] * F(j)) * r[k - j]
        r[k] = s / F(k)
    return r


def log1d(xs, n, seed):
    r = [ZERO] * n
    r[0] = F(seed)
    for k in range(1, n):
        if len(xs) == 1:
            continue
        s = ZERO
        for j in range(max(1, k + 1 - len(xs)), k):
            s = s + (xs[k - j] * r[j]) * F(j)
        xk = xs[k] if k < len(xs) else ZERO
        r[k] = ((xk * F(k) - s) / xs[0]) / F(k)
    return r


def _rows(a):
    a = np.asarray(a, dtype=np.float64)
    assert a.ndim == 2
    return [[F(v) for v in row] for row in a]


def _add(c, o):
    return [a + b for a, b in zip(c, o)]


def mul(x, y, n):
    n0, n1 = n
    x, y = _rows(x), _rows(y)
    with np.errstate(all="ignore"):
        z = [[ZERO] * n1 for _ in range(n0)]
        for k in range(n0):
            for j in range(max(0, k + 1 - len(y)), min(k + 1, len(x))):
                z[k] = _add(z[k], mul1d(x[j], y[k - j], n1))
    return np.array(z, dtype=np.float64).reshape(n0, n1)


def div(x, y, n):
    n0, n1 = n
    x, y = _rows(x), _rows(y)
    with np.errstate(all="ignore"):
        r = []
        for k in range(n0):
            c = [ZERO] * n1
            for j in range(max(0, k + 1 - len(y)), k):
                c = _add(c, mul1d(r[j], y[k - j], n1))
            c = [-v for v in c]
            if k < len(x):
                for i, v in enumerate(x[k]):
                    c[i] = c[i] + v
            r.append(div1d(c, y[0], n1))
    return np.array(r, dtype=np.float64).reshape(n0, n1)


def exp(x, n, seed=None):
    n0, n1 = n
    x = _rows(x)
    with np.errstate(all="ignore"):
        r = [exp1d(x[0], n1, math.exp(x[0][0]) if seed is None else seed)]
        for k in range(1, n0):
            c = [ZERO] * n1
            for j in range(1, min(len(x), k + 1)):
                c = _add(c, mul1d([v * F(j) for v in x[j]], r[k - j], n1))
            r.append([v / F(k) for v in c])
    return np.array(r, dtype=np.float64).reshape(n0, n1)


def log(x, n, seed=None):
    n0, n1 = n
    x = _rows(x)
    with np.errstate(all="ignore"):
        r = [log1d(x[0], n1, math.log(x[0][0]) if seed is None else seed)]
        for k in range(1, n0):
            c = [ZERO] * n1
            for j in range(max(1, k + 1 - len(x)), k):
                c = _add(c, mul1d(x[k - j], [v * F(j) for v in r[j]], n1))
            c = [-v for v in c]
            if k < len(x):
                for i, v in enumerate(x[k]):
                    c[i] = c[i] + F(k) * v
            c = div1d(c, x[0], n1)
            r.append([v / F(k) for v in c])
    return np.array(r, dtype=np.float64).reshape(n0, n1)
