"""The four trivariate recursions of genfer_amd.series3 (include/gftaylor.h) in plain Python, one IEEE operation at a time.

An item is a numpy float64 array ``[n0, n1, n2]``; the operands may be smaller (compact).  Two rules come before the loops, both
decided by the shapes alone.  Rule 1: the recursion runs on the stored result shape ``S`` (``result_shape``), not on ``n``, and
everything outside ``S`` is +0.0.  Rule 2: an ``S`` with unit axes is the item without them -- the rank-2 loops of
``_series2_model``, its rank-1 loops, or (three unit axes) those at one coefficient.  With every ``S_a >= 2`` the loops below run:
the terms of an output row ``(k0, k1)`` are the univariate products ``mul1d`` of two rows, each formed from 0.0 first and then added,
for ``j0`` ascending and inside it ``j1`` ascending, to the row's one accumulator; the slab steps of ``div`` / ``log`` are the
rank-2 division, slab 0 of ``exp`` / ``log`` the rank-2 recursion.  ``on``: the shape to compute on in place of ``S`` (the tests'
sentinel: computing on ``n`` is a different association)."""
import math

import numpy as np

import _series2_model as m2
from _series2_model import ZERO, F, mul1d


def result_shape(op, n, nx, ny=None):
    if op == "mul":
        return tuple(min(n[a], nx[a] + ny[a] - 1) for a in range(3))
    if op == "div":
        return tuple(nx[a] if ny[a] == 1 else n[a] for a in range(3))
    return tuple(1 if nx[a] == 1 else n[a] for a in range(3))


def _slabs(a):
    a = np.asarray(a, dtype=np.float64)
    assert a.ndim == 3
    return [[[F(v) for v in row] for row in slab] for slab in a]


def _zeros(n1, n2):
    return [[ZERO] * n2 for _ in range(n1)]


def _acc(c, a, b, n2):
    """c[k1] += mul1d(a[j1], b[k1 - j1]) for j1 ascending over the stored rows: the rank-2 product added into the accumulators"""
    for k1 in range(len(c)):
        for j1 in range(max(0, k1 + 1 - len(b)), min(k1 + 1, len(a))):
            c[k1] = [u + v for u, v in zip(c[k1], mul1d(a[j1], b[k1 - j1], n2))]


def _scaled(a, j):
    return [[v * F(j) for v in row] for row in a]


def _add_stored(c, xk, scale=None):
    for i, row in enumerate(xk):
        for l, v in enumerate(row):
            c[i][l] = c[i][l] + (v if scale is None else F(scale) * v)


def _mul3(x, y, s):
    x, y = _slabs(x), _slabs(y)
    z = []
    for k0 in range(s[0]):
        c = _zeros(s[1], s[2])
        for j0 in range(max(0, k0 + 1 - len(y)), min(k0 + 1, len(x))):
            _acc(c, x[j0], y[k0 - j0], s[2])
        z.append(c)
    return np.array(z, dtype=np.float64).reshape(s)


def _div3(x, y, s):
    x, y = _slabs(x), _slabs(y)
    r = []
    for k0 in range(s[0]):
        c = _zeros(s[1], s[2])
        for j0 in range(max(0, k0 + 1 - len(y)), k0):
            _acc(c, r[j0], y[k0 - j0], s[2])
        c = [[-v for v in row] for row in c]
        if k0 < len(x):
            _add_stored(c, x[k0])
        r.append([[F(v) for v in row] for row in m2.div(c, y[0], s[1:])])
    return np.array(r, dtype=np.float64).reshape(s)


def _exp3(x, s, seed):
    x = _slabs(x)
    r = [[[F(v) for v in row] for row in m2.exp(x[0], s[1:], seed)]]
    for k0 in range(1, s[0]):
        c = _zeros(s[1], s[2])
        for j0 in range(1, min(len(x), k0 + 1)):
            _acc(c, _scaled(x[j0], j0), r[k0 - j0], s[2])
        r.append([[v / F(k0) for v in row] for row in c])
    return np.array(r, dtype=np.float64).reshape(s)


def _log3(x, s, seed):
    x = _slabs(x)
    r = [[[F(v) for v in row] for row in m2.log(x[0], s[1:], seed)]]
    for k0 in range(1, s[0]):
        c = _zeros(s[1], s[2])
        for j0 in range(max(1, k0 + 1 - len(x)), k0):
            _acc(c, x[k0 - j0], _scaled(r[j0], j0), s[2])
        c = [[-v for v in row] for row in c]
        if k0 < len(x):
            _add_stored(c, x[k0], k0)
        c = m2.div(c, x[0], s[1:])
        r.append([[F(v) / F(k0) for v in row] for row in c])
    return np.array(r, dtype=np.float64).reshape(s)


def _run(op, x, y, n, seed, on):
    x = np.asarray(x, dtype=np.float64)
    y = None if y is None else np.asarray(y, dtype=np.float64)
    n = tuple(n)
    s = tuple(on) if on is not None else result_shape(op, n, x.shape, None if y is None else y.shape)
    keep = tuple(a for a in range(3) if s[a] != 1)  # rule 2: the unit axes of S are squeezed
    sq = tuple(s[a] for a in keep)
    xs = x.reshape(tuple(x.shape[a] for a in keep))
    ys = None if y is None else y.reshape(tuple(y.shape[a] for a in keep))
    if op in ("exp", "log") and seed is None:
        seed = (math.exp if op == "exp" else math.log)(x[0, 0, 0])
    with np.errstate(all="ignore"):
        if len(sq) == 3:
            core = {"mul": lambda: _mul3(xs, ys, sq), "div": lambda: _div3(xs, ys, sq), "exp": lambda: _exp3(xs, sq, seed),
                    "log": lambda: _log3(xs, sq, seed)}[op]()
        elif len(sq) == 2:
            core = getattr(m2, op)(xs, ys, sq) if ys is not None else getattr(m2, op)(xs, sq, seed)
        else:
            k = sq[0] if sq else 1
            xr = [F(v) for v in xs.reshape(-1)]
            yr = None if ys is None else [F(v) for v in ys.reshape(-1)]
            core = np.array({"mul": lambda: m2.mul1d(xr, yr, k), "div": lambda: m2.div1d(xr, yr, k), "exp": lambda: m2.exp1d(xr, k, seed),
                             "log": lambda: m2.log1d(xr, k, seed)}[op](), dtype=np.float64)
    out = np.zeros(n)
    out[:s[0], :s[1], :s[2]] = core.reshape(s)
    return out


def mul(x, y, n, on=None):
    return _run("mul", x, y, n, None, on)


def div(x, y, n, on=None):
    return _run("div", x, y, n, None, on)


def exp(x, n, seed=None, on=None):
    return _run("exp", x, None, n, seed, on)


def log(x, n, seed=None, on=None):
    return _run("log", x, None, n, seed, on)
