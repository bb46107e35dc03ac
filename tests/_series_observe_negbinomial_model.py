"""The negative-binomial observation (include/gftaylor.h: gft[i]_series_lah_row, gft[i]_series_observe_negbinomial and
gft[i]_series2_observe_negbinomial) in numpy: the stated loops, vectorised over the batch axes and sequential over the passes and
along the axis, with the arithmetic classes ``F64`` and ``IV`` of tests/_series_observe_model.py and ``mul_linear`` of
tests/_series_linear_model.py.  An F64 operand is ``[B..., item]`` with ``x`` and ``p`` ``[B...]`` and ``ls`` ``[B..., K + 1]``;
interval tensors carry the two planes in front.  ``axis`` is -1 or -2.  ``oracle_negbinomial`` is the reference's own sequence
(generating_function.rs:731-750) on the oracle's handle API, item by item."""
import numpy as np

import _series_linear_model as LM
from _series_observe_chain_model import _batched, _is, _lift, _where, result_shape  # noqa: F401
from _series_observe_model import F64, IV, _fmax, _fmin, factors  # noqa: F401

INF = np.inf


def _const(A, v, like):
    """the scalar v as an array of like's shape ([B...] or [2, B...])"""
    return np.full(np.shape(like), float(v))


def _sub(A, a, b):
    """interval.rs:148-155: a + (-b)"""
    if not A.planes:
        with np.errstate(all="ignore"):
            return a - b
    return A.add(a, np.stack([-b[1], -b[0]]))


def _div(A, a, b):
    """a / b elementwise; interval.rs:199-234 (IV.div of the observation model is its scalar form)"""
    with np.errstate(all="ignore"):
        if not A.planes:
            return a / b
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
        nan = np.isnan(a).any(axis=0) | np.isnan(b).any(axis=0)
        az, bz = (a[0] == 0.0) & (a[1] == 0.0), (b[0] == 0.0) & (b[1] == 0.0)
        b1 = (b[0] == 1.0) & (b[1] == 1.0)
        lo, hi = np.full(a[0].shape, INF), np.full(a[0].shape, -INF)
        cz = (b[0] <= 0.0) & (0.0 <= b[1])
        hi = np.where(cz & (0.0 <= a[0]), INF, hi)
        lo = np.where(cz & ~(0.0 <= a[0]), -INF, lo)
        lo = np.where(cz & (a[1] <= 0.0), -INF, lo)
        hi = np.where(cz & ~(a[1] <= 0.0), INF, hi)
        for v in (a[0] / b[0], a[0] / b[1], a[1] / b[0], a[1] / b[1]):
            lo, hi = _fmin(lo, v), _fmax(hi, v)
        g = IV._widen(lo, hi)
        g = np.where(b1, a, g)
        g = np.where(az & ~bz, a, g)
        return np.where(nan, np.nan, g)


def lah_row(A, p, order):
    """generating_function.rs:713-730: [B...] -> [B..., order + 1]; every multiplication by and addition of the absent entries'
    zero is performed"""
    p = np.asarray(p, dtype=np.float64)
    one, zero = _const(A, 1, p), _const(A, 0, p)
    one_mp = _sub(A, one, p)
    prev = [one]
    for d in range(1, order + 1):
        q = _div(A, one_mp, _const(A, d, p))
        nxt = []
        for i in range(d + 1):
            a = prev[i] if i < len(prev) else zero
            b = prev[i - 1] if 1 <= i <= len(prev) else zero
            nxt.append(A.mul(q, A.add(A.mul(a, _const(A, d + i - 1, p)), b)))
        prev = nxt
    return np.stack(prev, axis=-1)


def lah_row_floats(p, order):
    """the same recurrence on one plain Python float"""
    prev = [1.0]
    for d in range(1, order + 1):
        nxt = []
        for i in range(d + 1):
            a = prev[i] if i < len(prev) else 0.0
            b = prev[i - 1] if 1 <= i <= len(prev) else 0.0
            nxt.append((1.0 - p) / float(d) * (a * float(d + i - 1) + b))
        prev = nxt
    return prev


def scalars(A, x, p):
    """c, m of from(p) * var(v, x, d) per item: where p is one by value Mul returns var itself"""
    p1 = _is(A, p, 1.0)
    one = _const(A, 1, p)
    c = _where(A, p1, x, A.mul(p, x), 0)
    m = _where(A, p1, one, A.mul(p, one), 0)
    return c, m


def powers(A, c, m, K, d):
    """P_0 .. P_K as [B..., len_i] arrays, len_i = min(d, i + 1)"""
    one = _const(A, 1, c)
    P = [np.stack([one], axis=-1)]
    if K >= 1:
        P.append(np.stack([np.broadcast_to(c, one.shape), np.broadcast_to(m, one.shape)], axis=-1))
    for i in range(1, K):
        P.append(LM.mul_linear(A, P[i], 0, c, m, min(d, P[i].shape[-1] + 1), 1))
    return P


def observe_negbinomial(A, a, axis, x, p, ls, degree_p1, rank):
    """Returns the result with degree_p1 coefficients on `axis` (and min(other, degree_p1) on the other axis of a rank-2 item)."""
    a = np.asarray(a, dtype=np.float64)
    ls = np.asarray(ls, dtype=np.float64)
    d, K = degree_p1, ls.shape[-1] - 1
    D = np.array(np.moveaxis(a, axis, -1))  # the acted-on axis last; at rank 2 the other one is at -2
    L = D.shape[-1]
    assert K >= 0 and d >= 3 and d + K <= L
    if rank == 2:
        D = D[..., :min(D.shape[-2], d), :]
    D = D[..., :d + K]
    extra = rank - 1  # item axes of a slice along the last axis
    batch = D.shape[A.planes:D.ndim - rank]
    x, p = _batched(A.planes, x, batch), _batched(A.planes, p, batch)
    ls = _batched(A.planes, ls, batch, (K + 1,))
    c, m = scalars(A, x, p)
    pf = [_const(A, 1, m)]
    for j in range(d - 1):
        pf.append(A.mul(pf[j], m))
    P = powers(A, c, m, K, d)
    ff = factors(A, "derivative", 1, max(d + K - 1, 1))
    # in a rank-2 item whose lines are columns the product walks the rows, and every term passes through mul_1d's own zero
    columns = rank == 2 and axis == -2 and D.shape[-2] > 1
    zeros = np.zeros(D.shape[:-1])
    first = (Ellipsis,) + (0,) * rank  # the item's first element
    total = None
    for i in range(K + 1):
        S = [A.mul(D[..., j], _lift(A, pf[j], extra)) for j in range(d)]
        if i == 0:
            U = S
        elif i == 1:
            U = LM.mul_linear(A, np.stack(S, axis=-1), rank - 1, c, m, d, rank)
            U = [U[..., j] for j in range(d)]
        else:
            Pi, U = P[i], []
            n = Pi.shape[-1]
            for j in range(d):
                acc = zeros
                for k in range(max(0, j + 1 - n), min(j + 1, d)):
                    t = A.mul(S[k], _lift(A, Pi[..., j - k], extra))
                    acc = A.add(acc, A.add(zeros, t) if columns else t)
                U.append(acc if columns else A.add(zeros, acc))
        li = ls[..., i]
        l0, l1, ll = _is(A, li, 0.0), _is(A, li, 1.0), _lift(A, li, rank)
        U = np.stack([np.broadcast_to(u, zeros.shape) for u in U], axis=-1)
        V = _where(A, l1, U, A.mul(ll, U), rank)
        if i == 0:
            total = np.array(_where(A, l0, np.zeros(V.shape), V, rank))
            total[first] = A.add(total[first], np.zeros(total[first].shape))
        else:
            full = A.add(A.add(np.zeros(V.shape), total), V)
            head = np.array(total)
            head[first] = A.add(total[first], np.zeros(total[first].shape))
            total = np.array(_where(A, l0, head, full, rank))
        if i < K:
            n = D.shape[-1] - 1
            D = np.stack([A.mul(D[..., j + 1], A.factor(ff[j], D.ndim - 1, axis)) for j in range(n)], axis=-1)
    return np.ascontiguousarray(np.moveaxis(total, -1, axis))


def oracle_lah_row(T, p, order, interval):
    """the interpreter's recurrence (gfh_genfun.hpp:554-565) on the oracle's scalars, through one-coefficient polynomials"""
    lead = 1 if interval else 0
    p = np.asarray(p, dtype=np.float64)
    flat = p.reshape(p.shape[:lead] + (-1,))
    outs = []
    for b in range(flat.shape[-1]):
        pb = (float(flat[0, b]), float(flat[1, b])) if interval else float(flat[b])
        S = T.from_scalar
        one_mp = S(1.0) - S(pb)
        prev = [S(1.0)]
        for d in range(1, order + 1):
            nxt = []
            for i in range(d + 1):
                a = prev[i] if i < len(prev) else S(0.0)
                bb = prev[i - 1] if 1 <= i <= len(prev) else S(0.0)
                nxt.append(one_mp / T.from_u32(d) * (a * T.from_u32(d + i - 1) + bb))
            prev = nxt
        outs.append(np.stack([np.asarray(q.array()).reshape((2,) if interval else ()) for q in prev], axis=-1))
    w = np.stack(outs, axis=lead)
    return w.reshape(p.shape + (order + 1,))


def oracle_negbinomial(T, a, item, var, x, p, ls, degree_p1, interval):
    """generating_function.rs:731-750 per item: a is [(2,) B..., item], x and p [(2,) B...], ls [(2,) B..., K + 1].  Returns the
    stacked stored arrays, which must have result_shape."""
    lead = 1 if interval else 0
    rank, d = len(item), degree_p1
    batch = a.shape[lead:a.ndim - rank]
    n = ls.shape[-1]
    flat = a.reshape(a.shape[:lead] + (-1,) + tuple(item))
    B = flat.shape[lead]
    xf = _batched(lead, x, batch).reshape(a.shape[:lead] + (B,))
    pf = _batched(lead, p, batch).reshape(a.shape[:lead] + (B,))
    lf = _batched(lead, ls, batch, (n,)).reshape(a.shape[:lead] + (B, n))
    sc = (lambda v, b: (float(v[0, b]), float(v[1, b]))) if interval else (lambda v, b: float(v[b]))
    want = ((2,) if interval else ()) + result_shape(item, var, d)
    outs = []
    for b in range(B):
        total = T.zero_with((d,) * rank)
        inner = T.new(flat[:, b] if interval else flat[b], item)
        pr = sc(pf, b)
        p_pow = T.one()
        p_pv = T.from_scalar(pr) * T.var(var, sc(xf, b), d)
        for i in range(n):
            subst = T.from_scalar(pr) * T.var_at_zero(var, d)
            total = total.add_scaled(inner.subst_var(var, subst) * p_pow, sc(lf[..., i], b))
            p_pow = p_pow * p_pv
            inner = inner.derivative(var, 1)
        arr = total.truncate_to_degree_p1(d).array()
        assert arr.shape == want, f"the oracle stores {arr.shape}, the definition {want} (item {b})"
        outs.append(arr)
    w = np.stack(outs, axis=lead)
    return w.reshape(w.shape[:lead] + batch + w.shape[lead + 1:])
