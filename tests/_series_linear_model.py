"""The batched affine substitutions (include/gftaylor.h: gft[i]_series_mul_linear / _compose_linear and their series2 twins) in
numpy: the stated loops, vectorised over the batch axes and sequential along the axis and over the steps, with the arithmetic classes
``F64`` and ``IV`` of tests/_series_observe_model.py.  An F64 operand is ``[B..., item]`` with ``c`` and ``m`` ``[B...]``; interval
tensors carry the two planes in front.  ``v`` and ``w`` are positions of an item's shape (rank 1: 0; rank 2: 0 is axis -2, 1 is axis
-1).  ``oracle_linear`` is the same call on the oracle's handle API, item by item."""
import numpy as np

from _series_observe_chain_model import _batched, _is, _lift, _where
from _series_observe_model import F64, IV  # noqa: F401


def compact_shape(op, item, v, w, n):
    """the stored shape of the definition: what the loops write, before the padding with +0.0 to n"""
    s = list(item)
    if op == "mul_linear":
        s[w] = min(n[w], item[w] + 1)
    elif w != v:
        s[v], s[w] = 1, min(n[w], item[w] + item[v] - 1)
    return tuple(s)


def default_order(op, item, v, w):
    """the order a call without n takes: the compact shape without truncation (mul_linear: one more on the axis), and never less than
    the operand's own shape -- for w != v that is f's length on v, of which index 0 alone is stored"""
    return tuple(max(k, s) for k, s in zip(compact_shape(op, item, v, w, tuple(k + sum(item) for k in item)), item))


def mul_linear(A, a, w, c, m, n_w, rank):
    """mt:611-623 on every line along w; compact: min(n_w, L + 1) on w"""
    a = np.asarray(a, dtype=np.float64)
    axis = w - rank
    src = np.moveaxis(a, axis, -1)
    L = src.shape[-1]
    keep = min(n_w, L + 1)
    extra = rank - 1
    batch = src.shape[A.planes:src.ndim - rank]
    c, m = _batched(A.planes, c, batch), _batched(A.planes, m, batch)
    c0, cl, ml = _is(A, c, 0.0), _lift(A, c, extra), _lift(A, m, extra)
    zeros = np.zeros(src.shape[:-1])
    out = []
    for j in range(keep):
        t = zeros if j == 0 else A.mul(src[..., j - 1], ml)
        if j < L:
            t = _where(A, c0, t, A.add(t, A.mul(cl, src[..., j])), extra)
        out.append(np.broadcast_to(t, zeros.shape))
    return np.ascontiguousarray(np.moveaxis(np.stack(out, axis=-1), -1, axis))


def compose_linear(A, f, v, c, m, w, n, rank):
    """x_v := c + m * x_w at the orders n (a tuple of `rank`); compact"""
    f = np.asarray(f, dtype=np.float64)
    vaxis = v - rank
    nfv = f.shape[vaxis]
    batch = f.shape[A.planes:f.ndim - rank]
    c, m = _batched(A.planes, c, batch), _batched(A.planes, m, batch)
    sl = lambda i: np.take(f, [i], axis=vaxis)  # noqa: E731  (slice i along v, the axis kept)
    res = A.add(np.zeros(sl(0).shape), sl(nfv - 1))
    for i in range(nfv - 2, -1, -1):
        res = np.array(mul_linear(A, res, w, c, m, n[w], rank))
        S = sl(i)
        idx = tuple(slice(0, k) for k in S.shape)
        res[idx] = A.add(res[idx], S)
    if w != v:
        return res
    # the power table where c == 0 (per item): slice i times p_i, p_0 = 1, p_{i+1} = p_i * m
    p, parts = np.ones(np.shape(m)), []
    for i in range(nfv):
        parts.append(A.mul(sl(i), _lift(A, p, rank)))
        p = A.mul(p, m)
    power = np.concatenate(parts, axis=vaxis)
    assert power.shape == res.shape
    return _where(A, _is(A, c, 0.0), power, res, rank)


def padded(A, res, n, rank):
    """the compact result inside +0.0 at the orders n"""
    out = np.zeros(res.shape[:res.ndim - rank] + tuple(n))
    out[tuple(slice(0, k) for k in res.shape)] = res
    return out


def oracle_linear(T, op, a, item, v, w, c, m, n, interval):
    """per item: mul_linear(c, m, w, stored shape, n) or subst_var(v, [c, m] on axis w) of the oracle; a is [(2,) B..., item], c and m
    [(2,) B...].  Returns the stacked stored arrays, which must have the definition's compact shape."""
    lead = 1 if interval else 0
    rank = len(item)
    batch = a.shape[lead:a.ndim - rank]
    flat = a.reshape(a.shape[:lead] + (-1,) + tuple(item))
    B = flat.shape[lead]
    cf = _batched(lead, c, batch).reshape(a.shape[:lead] + (B,))
    mf = _batched(lead, m, batch).reshape(a.shape[:lead] + (B,))
    sc = (lambda s, b: (float(s[0, b]), float(s[1, b]))) if interval else (lambda s, b: float(s[b]))
    want = ((2,) if interval else ()) + compact_shape(op, item, v, w, n)
    outs = []
    for b in range(B):
        p = T.new(flat[:, b] if interval else flat[b], n)
        if op == "mul_linear":
            r = p.mul_linear(sc(cf, b), sc(mf, b), w, want[lead:], n)
        else:
            lin = np.stack([cf[..., b], mf[..., b]], axis=-1)  # [(2,) 2]
            sshape = tuple(2 if k == w else 1 for k in range(rank))
            r = p.subst_var(v, T.new(lin.reshape(a.shape[:lead] + sshape), n))
        arr = r.array()
        assert arr.shape == want, f"the oracle stores {arr.shape}, the definition {want} (item {b})"
        outs.append(arr)
    s = np.stack(outs, axis=lead)
    return s.reshape(s.shape[:lead] + batch + s.shape[lead + 1:])
