"""The four trivariate recursions of genfer_amd.interval_series3 (include/gftaylor.h): the loops of tests/_series3_model.py with every
scalar step ONE operation of the oracle's Interval (orci_scalar_op through tests/_series2_interval_model.Ops).

An item is a numpy float64 array ``[2, n0, n1, n2]`` = (lo, hi); the operands may be smaller (compact).  Both rules come before the
loops, as at f64: the recursion runs on the stored result shape ``S`` (``_series3_model.result_shape``) with ``[+0.0, +0.0]`` outside
it, and an ``S`` with unit axes is the item without them -- the rank-2 loops of ``_series2_interval_model``, its rank-1 loops, or
those at one coefficient.  ``j0`` and ``k0`` enter as the point intervals ``from_u32`` where the oracle's ``exp_rec`` / ``log_rec`` put
them.  ``on``: the shape to compute on in place of ``S``; ``squeeze=False``: the rank-3 loops in the caller's axis order whatever
unit axes the shape has (the tests' two sentinels).  Every step is a ctypes call: items of at most a few hundred coefficients."""
import numpy as np

import _series2_interval_model as m2
from _series2_interval_model import ZERO, Ops, mul1d  # noqa: F401  (Ops re-exported)
from _series3_model import result_shape


def _slabs(a):
    a = np.asarray(a, dtype=np.float64)
    assert a.ndim == 4 and a.shape[0] == 2
    return [[[(float(a[0, i, j, k]), float(a[1, i, j, k])) for k in range(a.shape[3])] for j in range(a.shape[2])] for i in range(a.shape[1])]


def _arr(slabs, s):
    """nested lists of (lo, hi) of shape s -> [2, s0, s1, s2]"""
    return np.array(slabs, dtype=np.float64).reshape(tuple(s) + (2,)).transpose(3, 0, 1, 2).copy()


def _rows2(slab):
    """a slab (rows of (lo, hi)) as the [2, n1, n2] array the rank-2 model takes"""
    return np.array(slab, dtype=np.float64).reshape(len(slab), len(slab[0]), 2).transpose(2, 0, 1)


def _back2(a):
    """[2, n1, n2] -> rows of (lo, hi)"""
    return [[(float(a[0, i, j]), float(a[1, i, j])) for j in range(a.shape[2])] for i in range(a.shape[1])]


def _zeros(n1, n2):
    return [[ZERO] * n2 for _ in range(n1)]


def _acc(o, c, a, b, n2):
    """c[k1] += mul1d(a[j1], b[k1 - j1]) for j1 ascending over the stored rows: each row sum formed from [0,0] first, then added"""
    for k1 in range(len(c)):
        for j1 in range(max(0, k1 + 1 - len(b)), min(k1 + 1, len(a))):
            c[k1] = [o.add(u, v) for u, v in zip(c[k1], mul1d(o, a[j1], b[k1 - j1], n2))]


def _mul3(o, x, y, s):
    x, y = _slabs(x), _slabs(y)
    z = []
    for k0 in range(s[0]):
        c = _zeros(s[1], s[2])
        for j0 in range(max(0, k0 + 1 - len(y)), min(k0 + 1, len(x))):
            _acc(o, c, x[j0], y[k0 - j0], s[2])
        z.append(c)
    return _arr(z, s)


def _div3(o, x, y, s):
    x, y = _slabs(x), _slabs(y)
    r = []
    for k0 in range(s[0]):
        c = _zeros(s[1], s[2])
        for j0 in range(max(0, k0 + 1 - len(y)), k0):
            _acc(o, c, r[j0], y[k0 - j0], s[2])
        c = [[o.neg(v) for v in row] for row in c]
        if k0 < len(x):
            for i, row in enumerate(x[k0]):
                for l, v in enumerate(row):
                    c[i][l] = o.add(c[i][l], v)
        r.append(_back2(m2.div(o, _rows2(c), _rows2(y[0]), s[1:])))
    return _arr(r, s)


def _exp3(o, x, s, seed):
    x = _slabs(x)
    r = [_back2(m2.exp(o, _rows2(x[0]), s[1:], seed))]
    for k0 in range(1, s[0]):
        c = _zeros(s[1], s[2])
        for j0 in range(1, min(len(x), k0 + 1)):
            _acc(o, c, [[o.mul(v, o.u(j0)) for v in row] for row in x[j0]], r[k0 - j0], s[2])
        r.append([[o.div(v, o.u(k0)) for v in row] for row in c])
    return _arr(r, s)


def _log3(o, x, s, seed):
    x = _slabs(x)
    r = [_back2(m2.log(o, _rows2(x[0]), s[1:], seed))]
    for k0 in range(1, s[0]):
        c = _zeros(s[1], s[2])
        for j0 in range(max(1, k0 + 1 - len(x)), k0):
            _acc(o, c, x[k0 - j0], [[o.mul(v, o.u(j0)) for v in row] for row in r[j0]], s[2])
        c = [[o.neg(v) for v in row] for row in c]
        if k0 < len(x):
            for i, row in enumerate(x[k0]):
                for l, v in enumerate(row):
                    c[i][l] = o.add(c[i][l], o.mul(o.u(k0), v))
        c = _back2(m2.div(o, _rows2(c), _rows2(x[0]), s[1:]))
        r.append([[o.div(v, o.u(k0)) for v in row] for row in c])
    return _arr(r, s)


def _run(o, op, x, y, n, seed, on, squeeze):
    x = np.asarray(x, dtype=np.float64)
    y = None if y is None else np.asarray(y, dtype=np.float64)
    n = tuple(n)
    s = tuple(on) if on is not None else result_shape(op, n, x.shape[1:], None if y is None else y.shape[1:])
    keep = tuple(a for a in range(3) if s[a] != 1) if squeeze else (0, 1, 2)  # rule 2: the unit axes of S are squeezed
    sq = tuple(s[a] for a in keep)
    xs = x.reshape((2,) + tuple(x.shape[1 + a] for a in keep))
    ys = None if y is None else y.reshape((2,) + tuple(y.shape[1 + a] for a in keep))
    if op in ("exp", "log"):
        assert seed is not None, "the interval seed of coefficient [0, 0, 0] (the caller forms it with the oracle's scalar exp / log)"
        seed = (float(seed[0]), float(seed[1]))
    if len(sq) == 3:
        core = {"mul": lambda: _mul3(o, xs, ys, sq), "div": lambda: _div3(o, xs, ys, sq), "exp": lambda: _exp3(o, xs, sq, seed),
                "log": lambda: _log3(o, xs, sq, seed)}[op]()
    elif len(sq) == 2:
        core = getattr(m2, op)(o, xs, ys, sq) if ys is not None else getattr(m2, op)(o, xs, sq, seed)
    else:
        k = sq[0] if sq else 1
        row = lambda a: [(float(l), float(h)) for l, h in zip(a[0].reshape(-1), a[1].reshape(-1))]  # noqa: E731
        xr, yr = row(xs), None if ys is None else row(ys)
        core = {"mul": lambda: m2.mul1d(o, xr, yr, k), "div": lambda: m2.div1d(o, xr, yr, k), "exp": lambda: m2.exp1d(o, xr, k, seed),
                "log": lambda: m2.log1d(o, xr, k, seed)}[op]()
        core = np.array(core, dtype=np.float64).reshape(k, 2).T
    out = np.zeros((2,) + n)
    out[:, :s[0], :s[1], :s[2]] = np.asarray(core).reshape((2,) + s)
    return out


def mul(o, x, y, n, on=None, squeeze=True):
    return _run(o, "mul", x, y, n, None, on, squeeze)


def div(o, x, y, n, on=None, squeeze=True):
    return _run(o, "div", x, y, n, None, on, squeeze)


def exp(o, x, n, seed, on=None, squeeze=True):
    return _run(o, "exp", x, None, n, seed, on, squeeze)


def log(o, x, n, seed, on=None, squeeze=True):
    return _run(o, "log", x, None, n, seed, on, squeeze)
