"""The batched observation ops (include/gftaylor.h: gft_series_* / gft_series2_* derivative, taylor_expansion_of_coeff, shift_down,
evaluate_all_one and their gfti_ twins) in numpy: the stated loops, vectorised over the leading (batch) axes and sequential along the
axis an operation acts on, so every coefficient has the bits the loops give.

``F64`` and ``IV`` are the two arithmetics.  An F64 operand is ``[B..., item]``; an interval operand is ``[2, B..., item]`` = (lo, hi)
and every step is one operation of the reference's Interval (round to nearest, one ulp outwards, its short-circuits).  ``axis`` is
-1 or -2, counted from the end, so the same code serves both layouts.  The adjoints at the end are the backward formulas of the
autograd functions (F64 only)."""
import numpy as np

INF = np.inf


def _quiet(f):
    def g(*a, **k):
        with np.errstate(all="ignore"):
            return f(*a, **k)
    return g


class F64:
    planes = 0

    @staticmethod
    def const(v):
        return np.float64(v)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape)

    add = staticmethod(_quiet(lambda a, b: a + b))
    mul = staticmethod(_quiet(lambda a, b: a * b))
    div = staticmethod(_quiet(lambda a, b: a / b))

    @staticmethod
    def factor(f, like_ndim, axis):
        return f


def next_up(x):
    """f64.rs:127-171 (gft_elem.hpp): the next double above; -0.0 counts as +0.0, NaN and +inf stay"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = np.atleast_1d(x + 0.0)
        bits = t.view(np.int64)
        r = (bits + ((bits >> 63) | 1)).view(np.float64)
        return np.where(t < INF, r, np.atleast_1d(x)).reshape(x.shape)


def next_down(x):
    return -next_up(-np.asarray(x, dtype=np.float64))


def _fmin(a, b):
    return np.where(a < b, a, b)


def _fmax(a, b):
    return np.where(a > b, a, b)


class IV:
    """interval.rs; an interval array is [2, ...]"""
    planes = 1

    @staticmethod
    def const(v):
        return np.array([float(v), float(v)])

    @staticmethod
    def zeros(shape):
        return np.zeros(shape)

    @staticmethod
    def _widen(lo, hi):
        return np.stack([next_down(lo), next_up(hi)])

    @staticmethod
    @_quiet
    def add(a, b):  # :126-139
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
        za, zb = (a[0] == 0.0) & (a[1] == 0.0), (b[0] == 0.0) & (b[1] == 0.0)
        g = IV._widen(a[0] + b[0], a[1] + b[1])
        return np.where(za, b, np.where(zb, a, g))

    @staticmethod
    @_quiet
    def mul(a, b):  # :164-190
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
        fin = lambda v: ((v[0] - v[0]) == 0.0) & ((v[1] - v[1]) == 0.0)  # noqa: E731
        pt = lambda v, c: (v[0] == c) & (v[1] == c)  # noqa: E731
        p, q, r, s = a[0] * b[0], a[0] * b[1], a[1] * b[0], a[1] * b[1]
        g = IV._widen(_fmin(_fmin(_fmin(p, q), r), s), _fmax(_fmax(_fmax(p, q), r), s))
        g = np.where(pt(b, -1.0), np.stack([-a[1], -a[0]]), g)
        g = np.where(pt(a, -1.0), np.stack([-b[1], -b[0]]), g)
        g = np.where(pt(b, 1.0), a, g)
        g = np.where(pt(a, 1.0), b, g)
        z = (pt(a, 0.0) & fin(b)) | (fin(a) & pt(b, 0.0))
        return np.where(z, 0.0, g)

    @staticmethod
    @_quiet
    def div(a, b):  # :199-234, scalars (the factor tables)
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert a.shape == (2,) and b.shape == (2,)
        if np.isnan(a).any() or np.isnan(b).any():
            return np.array([np.nan, np.nan])
        if a[0] == 0.0 and a[1] == 0.0 and not (b[0] == 0.0 and b[1] == 0.0):
            return a
        if b[0] == 1.0 and b[1] == 1.0:
            return a
        lo, hi = INF, -INF
        if b[0] <= 0.0 <= b[1]:
            if 0.0 <= a[0]:
                hi = INF
            else:
                lo = -INF
            if a[1] <= 0.0:
                lo = -INF
            else:
                hi = INF
        for v in (a[0] / b[0], a[0] / b[1], a[1] / b[0], a[1] / b[1]):
            lo = lo if lo < v else v
            hi = hi if hi > v else v
        return np.array([float(next_down(lo)), float(next_up(hi))])

    @staticmethod
    def factor(f, like_ndim, axis):
        """a scalar interval [2] against an array [2, ...]: the planes stay in front"""
        return np.asarray(f).reshape((2,) + (1,) * (like_ndim - 1))


def factors(A, op, k, m):
    """the running-product table of (op, k, m): k_factor_table's loops (mt:472-478, 499-506)"""
    out = []
    if op == "derivative":
        ff = A.const(1)
        for i in range(1, k + 1):
            ff = A.mul(ff, A.const(i))
        for j in range(m):
            out.append(ff)
            ff = A.mul(ff, A.div(A.const(k + j + 1), A.const(j + 1)))
    else:
        f = A.const(1)
        out.append(f)
        for j in range(1, m):
            f = A.mul(f, A.div(A.const(k + j), A.const(j)))
            out.append(f)
    return out


def _scaled(A, op, x, axis, k):
    x = np.asarray(x, dtype=np.float64)
    m = x.shape[axis] - k
    assert 0 <= k < x.shape[axis]
    fs = factors(A, op, k, m)
    out = np.array(np.moveaxis(x, axis, -1)[..., k:])  # the acted-on axis last
    for j in range(m):
        if op != "derivative" and j == 0:
            continue  # slice 0 is copied untouched
        sl = out[..., j]
        out[..., j] = A.mul(sl, A.factor(fs[j], sl.ndim, axis))
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))


def derivative(A, x, axis, k):
    return _scaled(A, "derivative", x, axis, k)


def taylor_expansion_of_coeff(A, x, axis, k):
    return _scaled(A, "coeff", x, axis, k)


def ordered_sum(A, x, cnt, fold8):
    """the sum of x[..., :cnt] along the LAST axis in ndarray's order: ascending from 0.0, or the 8-way unrolled fold"""
    acc = A.zeros(x.shape[:-1])
    i = 0
    if fold8:
        p = [A.zeros(x.shape[:-1]) for _ in range(8)]
        while cnt - i >= 8:
            for u in range(8):
                p[u] = A.add(p[u], x[..., i + u])
            i += 8
        for u in range(4):
            acc = A.add(acc, A.add(p[u], p[u + 4]))
    for j in range(i, cnt):
        acc = A.add(acc, x[..., j])
    return acc


def shift_down(A, x, axis, k, rank):
    """rank: 1 or 2 -- ndarray folds a unit-stride axis of a rank-2 array 8-way (axis -1, or axis -2 of a one-column item)"""
    x = np.asarray(x, dtype=np.float64)
    ln = x.shape[axis]
    assert 0 <= k < ln
    fold8 = rank == 2 and (axis == -1 or x.shape[-1] == 1)
    xl = np.moveaxis(x, axis, -1)
    out = np.array(xl[..., k:])
    if ln == k + 1:
        out[..., 0] = ordered_sum(A, xl, ln, fold8)
    else:
        out[..., 0] = A.add(xl[..., k], ordered_sum(A, xl, k, fold8))
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))


def evaluate_all_one(A, x, rank):
    """0.0 + x[0] + x[1] + ... over the item in row-major order (mt:583-586)"""
    x = np.asarray(x, dtype=np.float64)
    flat = x.reshape(x.shape[:x.ndim - rank] + (-1,))
    return ordered_sum(A, flat, flat.shape[-1], False)


# ---- the adjoints (F64): the backward passes of the autograd functions ------------------------------------------------------------


def scaled_adj(op, g, axis, k):
    """gx[k + j] = g[j] * factor_j, gx[< k] = +0.0"""
    g = np.moveaxis(np.asarray(g, dtype=np.float64), axis, -1)
    m = g.shape[-1]
    fs = np.array(factors(F64, op, k, m))
    gx = np.zeros(g.shape[:-1] + (k + m,))
    gx[..., k:] = g * fs
    return np.ascontiguousarray(np.moveaxis(gx, -1, axis))


def shift_down_adj(g, axis, k):
    """gx[i] = g[0] for i <= k, gx[k + j] = g[j] for j >= 1"""
    g = np.moveaxis(np.asarray(g, dtype=np.float64), axis, -1)
    gx = np.concatenate([np.repeat(g[..., :1], k, axis=-1), g], axis=-1)
    return np.ascontiguousarray(np.moveaxis(gx, -1, axis))


def evaluate_all_one_adj(g, item_shape):
    g = np.asarray(g, dtype=np.float64)
    return np.broadcast_to(g[(...,) + (None,) * len(item_shape)], g.shape + tuple(item_shape)).copy()
