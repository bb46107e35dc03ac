"""What a zero-pattern claim of the interval handle API means, in plain numpy.

The library's `Support` (gft_api.hip) says where a tensor holds coefficients that are exactly [0,0].  `claim_holds` checks such a
claim against the two planes of a tensor; `proves_nonlinear` restates what a consumer concludes from it."""
import numpy as np

ZAX = 8               # Buf::ZAX: the axes a claim can speak about
UNBOUNDED = 0xFFFFFFFF  # h[u] of an axis the box does not end on

UNKNOWN, MEASURED_IRREGULAR, NO_ZERO, LEADING_SLABS, PADDED_BOX, ALL_ZERO = range(6)
INFORMATIVE = (NO_ZERO, LEADING_SLABS, PADDED_BOX, ALL_ZERO)


def zero_mask(lo, hi):
    """True where the interval is exactly [0,0] (-0.0 counts: iv:100-103 compares with ==)."""
    return (np.asarray(lo) == 0.0) & (np.asarray(hi) == 0.0)


def _first(bad):
    idx = np.argwhere(bad)
    return tuple(int(i) for i in idx[0]) if len(idx) else None


def claim_holds(kind, z, h, lo, hi):
    """None if the claim (kind, z[8], h[8]) is true of the tensor with planes lo / hi, else (index, reason) of the first
    counter-example.  Axes the tensor does not have count as extent 1."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    zm = zero_mask(lo, hi)
    shape = lo.shape
    if kind in (UNKNOWN, MEASURED_IRREGULAR):
        return None
    if kind == NO_ZERO:
        i = _first(zm)
        return None if i is None else (i, "claimed free of exact zeros, holds one")
    if kind == ALL_ZERO:
        i = _first(~zm)
        return None if i is None else (i, "claimed all zero, holds something else")
    idx = np.indices(shape) if len(shape) else np.zeros((0,), dtype=int)
    if kind == LEADING_SLABS:  # [0,0] iff k_u < z[u] for some u
        slab = np.zeros(shape, dtype=bool)
        for u in range(ZAX):
            slab |= (idx[u] < z[u]) if u < len(shape) else (0 < z[u])
        i = _first(slab != zm)
        return None if i is None else (i, "in a claimed zero slab but not zero" if slab[i] else "zero outside the claimed slabs")
    if kind == PADDED_BOX:
        # zero outside z[u] <= k_u < h[u] — and nowhere inside: sum_support's box_of takes the box as the operand's NON-ZERO
        # coefficients (a box that fills the sum makes it "no zero", a union of boxes becomes "exactly the leading slabs")
        inside = np.ones(shape, dtype=bool)
        for u in range(ZAX):
            inside &= ((idx[u] >= z[u]) & (idx[u] < h[u])) if u < len(shape) else bool(z[u] <= 0 < h[u])
        i = _first(inside == zm)
        return None if i is None else (i, "zero inside the claimed box" if inside[i] else "outside the claimed box but not zero")
    return ((), f"unknown claim kind {kind}")


def proves_nonlinear(kind, z, shape):
    """support_proves_nonlinear: a tensor with this claim cannot be c + m * x_v (so no scan is launched)."""
    if kind not in (NO_ZERO, LEADING_SLABS):
        return False
    return any(n >= 3 for n in shape) or sum(1 for n in shape if n == 2) >= 2

