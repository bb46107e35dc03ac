"""The fused observation chain (include/gftaylor.h: gft[i]_series_observe_chain / gft[i]_series2_observe_chain) in numpy: the stated
loops in their general form (dl and lout are computed, not assumed), vectorised over the batch axes and sequential over the steps
and along the axis, with the arithmetic classes ``F64`` and ``IV`` of tests/_series_observe_model.py.  An F64 operand is
``[B..., item]`` with ``x`` ``[B...]`` and ``cs`` ``[B..., nsteps]``; interval tensors carry the two planes in front.  ``axis`` is
-1 or -2.  ``oracle_chain`` is the same call on the oracle's handle API, item by item."""
import numpy as np

from _series_observe_model import F64, IV, factors  # noqa: F401


def _batched(planes, v, batch, tail=()):
    """x or cs broadcast to the batch: missing batch axes go in front -- behind the plane axis of an interval tensor, which stays first"""
    v = np.asarray(v, dtype=np.float64)
    full = planes + len(batch) + len(tail)
    if planes and v.ndim < full:
        v = v[(slice(None),) + (None,) * (full - v.ndim)]
    return np.broadcast_to(v, ((2,) if planes else ()) + tuple(batch) + tuple(tail))


def _lift(A, v, extra):
    """a per-item value ([B...] or [2, B...]) against slices with `extra` item axes behind the batch"""
    v = np.asarray(v)
    return v[(Ellipsis,) + (None,) * extra]


def _is(A, v, c):
    """the scalar test of the loops: the value equals c (-0.0 == 0.0); an interval when both bounds do.  [B...]"""
    v = np.asarray(v, dtype=np.float64)
    return (v[0] == c) & (v[1] == c) if A.planes else v == c


def _where(A, mask, a, b, extra):
    """per item: a where mask else b; mask is [B...]"""
    m = mask[(Ellipsis,) + (None,) * extra]
    if A.planes:
        m = m[None]
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    shape = np.broadcast_shapes(m.shape, a.shape, b.shape)
    return np.where(np.broadcast_to(m, shape), np.broadcast_to(a, shape), np.broadcast_to(b, shape))


def observe_chain(A, a, axis, x, cs, degree_p1, rank):
    """x None: the continuous form.  Returns the result with degree_p1 coefficients on `axis`."""
    a = np.asarray(a, dtype=np.float64)
    nsteps = np.shape(cs)[-1]
    src = np.array(np.moveaxis(a, axis, -1))  # the acted-on axis last; at rank 2 the other one is at -2
    L0 = src.shape[-1]
    assert degree_p1 >= 2 and nsteps >= 1 and degree_p1 + nsteps <= L0
    extra = rank - 1  # item axes of a slice along the last axis
    batch = src.shape[A.planes:src.ndim - rank]
    one = A.const(1)
    dead = np.zeros(batch, dtype=bool)
    cs = _batched(A.planes, cs, batch, (nsteps,))
    if x is not None:
        x = _batched(A.planes, x, batch)
        x0, x1, xs = _is(A, x, 0.0), _is(A, x, 1.0), _lift(A, x, extra)
    for t in range(nsteps):
        d = degree_p1 + (nsteps - 1 - t)
        if rank == 2:
            src = src[..., :min(src.shape[-2], d), :]
        L = src.shape[-1]
        dl = min(L - 1, d)
        ff = factors(A, "derivative", 1, max(dl, 1))
        c = cs[..., t]
        c0, c1, cl = _is(A, c, 0.0), _is(A, c, 1.0), _lift(A, c, extra)
        D = [A.mul(src[..., j + 1], A.factor(ff[j], src.ndim - 1, axis)) for j in range(dl)]
        zeros = np.zeros(src.shape[:-1])
        f1 = A.factor(one, src.ndim - 1, axis)
        out = []
        if x is not None:
            lout = min(dl + 1, d)
            for kv in range(lout):
                lo1 = A.mul(D[kv - 1], f1) if 1 <= kv <= dl else zeros
                res = A.add(zeros, lo1)
                if kv < dl:
                    res = A.add(res, _where(A, x1, D[kv], A.mul(xs, D[kv]), extra))
                res = _where(A, x0, zeros if kv == 0 else A.mul(D[kv - 1], f1), res, extra)
                res = _where(A, c1, res, A.mul(cl, res), extra)
                out.append(_where(A, c0, zeros, res, extra))
        else:
            for kv in range(dl):
                res = _where(A, c1, D[kv], A.mul(cl, D[kv]), extra)
                out.append(_where(A, c0, zeros, res, extra))
        dead = dead | c0
        src = np.stack(out, axis=-1)
        src = _where(A, dead, np.zeros(src.shape), src, rank)  # c == 0: the item is all +0.0 from here on
    assert src.shape[-1] == degree_p1
    return np.ascontiguousarray(np.moveaxis(src, -1, axis))


def result_shape(item, var, degree_p1):
    if len(item) == 1:
        return (degree_p1,)
    return (degree_p1, min(item[1], degree_p1)) if var == 0 else (min(item[0], degree_p1), degree_p1)


def oracle_chain(T, a, item, var, x, cs, degree_p1, interval):
    """the oracle's observe_chain (x None: derive_scale step by step) per item; a is [(2,) B..., item], x [(2,) B...], cs [(2,) B..., n].
    Returns the stacked stored arrays, which must have result_shape -- the oracle stores less where its Mul takes a shortcut."""
    lead = 1 if interval else 0
    rank = len(item)
    batch = a.shape[lead:a.ndim - rank]
    n = cs.shape[-1]
    flat = a.reshape(a.shape[:lead] + (-1,) + tuple(item))
    B = flat.shape[lead]
    xf = None if x is None else _batched(lead, x, batch).reshape(a.shape[:lead] + (B,))
    cf = _batched(lead, cs, batch, (n,)).reshape(a.shape[:lead] + (B, n))
    sc = (lambda v, b: (float(v[0, b]), float(v[1, b]))) if interval else (lambda v, b: float(v[b]))
    outs = []
    for b in range(B):
        p = T.new(flat[:, b] if interval else flat[b], item)
        steps = [sc(cf[..., t], b) for t in range(n)]
        if x is not None:
            r = p.observe_chain(var, sc(xf, b), steps, degree_p1)
        else:
            r = p
            for t in range(n):
                r = r.derive_scale(var, steps[t], degree_p1 + (n - 1 - t))
        arr = r.array()
        want = ((2,) if interval else ()) + result_shape(item, var, degree_p1)
        assert arr.shape == want, f"the oracle stores {arr.shape}, the definition {want} (item {b})"
        outs.append(arr)
    w = np.stack(outs, axis=lead)
    return w.reshape(w.shape[:lead] + batch + w.shape[lead + 1:])
