"""The four bivariate recursions of genfer_amd.interval_series2 (include/gftaylor.h): the loops of tests/_series2_model.py with every
scalar step ONE operation of the oracle's Interval (orci_scalar_op: add 0, sub 1, mul 2, div 3, neg 4).

An item is a numpy float64 array ``[2, n0, n1]`` = (lo, hi); the operands may be smaller (compact).  Every step is a ctypes call,
so this is for items of at most about 20 coefficients.  ``j`` and ``k`` enter as the point intervals ``[j, j]``, ``[k, k]``
(``Interval::from_u32``) at the places the oracle's ``exp_1d`` / ``exp_rec`` / ``log_1d`` / ``log_rec`` put them; ``log1d`` of a
one-coefficient row stores [0,0] above coefficient 0, as ``gfti_series_log`` does."""
import ctypes as C

import numpy as np

D2 = C.c_double * 2
ZERO = (0.0, 0.0)


class Ops:
    def __init__(self, oracle_lib):
        self.f = oracle_lib.orci_scalar_op

    def _op(self, code, a, b=None):
        out = D2()
        assert self.f(code, D2(float(a[0]), float(a[1])), None if b is None else D2(float(b[0]), float(b[1])), out) == 0
        return (out[0], out[1])

    def add(self, a, b):
        return self._op(0, a, b)

    def sub(self, a, b):
        return self._op(1, a, b)

    def mul(self, a, b):
        return self._op(2, a, b)

    def div(self, a, b):
        return self._op(3, a, b)

    def neg(self, a):
        return self._op(4, a)

    @staticmethod
    def u(j):
        return (float(j), float(j))


def mul1d(o, xs, ys, n):
    zs = [ZERO] * n
    for k in range(n):
        s = ZERO
        for j in range(max(0, k + 1 - len(ys)), min(k + 1, len(xs))):
            s = o.add(s, o.mul(xs[j], ys[k - j]))
        zs[k] = s
    return zs


def div1d(o, xs, ys, n):
    r = [ZERO] * n
    for k in range(n):
        s = ZERO
        for j in range(max(0, k + 1 - len(ys)), k):
            s = o.add(s, o.mul(r[j], ys[k - j]))
        c = o.neg(s)
        if k < len(xs):
            c = o.add(c, xs[k])
        r[k] = o.div(c, ys[0])
    return r


def exp1d(o, xs, n, seed):
    r = [ZERO] * n
    r[0] = tuple(seed)
    for k in range(1, n):
        s = ZERO
        for j in range(1, min(len(xs), k + 1)):
            s = o.add(s, o.mul(o.mul(xs[j], o.u(j)), r[k - j]))
        r[k] = o.div(s, o.u(k))
    return r


def log1d(o, xs, n, seed):
    r = [ZERO] * n
    r[0] = tuple(seed)
    for k in range(1, n):
        if len(xs) == 1:
            continue
        s = ZERO
        for j in range(max(1, k + 1 - len(xs)), k):
            s = o.add(s, o.mul(o.mul(xs[k - j], r[j]), o.u(j)))
        xk = xs[k] if k < len(xs) else ZERO
        r[k] = o.div(o.div(o.sub(o.mul(xk, o.u(k)), s), xs[0]), o.u(k))
    return r


def _rows(a):
    a = np.asarray(a, dtype=np.float64)
    assert a.ndim == 3 and a.shape[0] == 2
    return [[(float(a[0, i, j]), float(a[1, i, j])) for j in range(a.shape[2])] for i in range(a.shape[1])]


def _out(rows, n):
    return np.array(rows, dtype=np.float64).reshape(n[0], n[1], 2).transpose(2, 0, 1).copy()


def _add(o, c, s):
    return [o.add(a, b) for a, b in zip(c, s)]


def mul(o, x, y, n):
    n0, n1 = n
    x, y = _rows(x), _rows(y)
    z = [[ZERO] * n1 for _ in range(n0)]
    for k in range(n0):
        for j in range(max(0, k + 1 - len(y)), min(k + 1, len(x))):
            z[k] = _add(o, z[k], mul1d(o, x[j], y[k - j], n1))
    return _out(z, n)


def div(o, x, y, n):
    n0, n1 = n
    x, y = _rows(x), _rows(y)
    r = []
    for k in range(n0):
        c = [ZERO] * n1
        for j in range(max(0, k + 1 - len(y)), k):
            c = _add(o, c, mul1d(o, r[j], y[k - j], n1))
        c = [o.neg(v) for v in c]
        if k < len(x):
            for i, v in enumerate(x[k]):
                c[i] = o.add(c[i], v)
        r.append(div1d(o, c, y[0], n1))
    return _out(r, n)


def exp(o, x, n, seed):
    n0, n1 = n
    x = _rows(x)
    r = [exp1d(o, x[0], n1, seed)]
    for k in range(1, n0):
        c = [ZERO] * n1
        for j in range(1, min(len(x), k + 1)):
            c = _add(o, c, mul1d(o, [o.mul(v, o.u(j)) for v in x[j]], r[k - j], n1))
        r.append([o.div(v, o.u(k)) for v in c])
    return _out(r, n)


def log(o, x, n, seed):
    n0, n1 = n
    x = _rows(x)
    r = [log1d(o, x[0], n1, seed)]
    for k in range(1, n0):
        c = [ZERO] * n1
        for j in range(max(1, k + 1 - len(x)), k):
            c = _add(o, c, mul1d(o, x[k - j], [o.mul(v, o.u(j)) for v in r[j]], n1))
        c = [o.neg(v) for v in c]
        if k < len(x):
            for i, v in enumerate(x[k]):
                c[i] = o.add(c[i], o.mul(o.u(k), v))
        c = div1d(o, c, x[0], n1)
        r.append([o.div(v, o.u(k)) for v in c])
    return _out(r, n)
