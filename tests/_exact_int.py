"""Exact integer helpers for the exact-tree tests (test_fuzz_exact_gpu.py): a plain integer truncated multivariate
product, and the project's own crossover arithmetic restated on shapes.  Nothing here calls the oracle or the library."""
import numpy as np

LIMIT = 2 ** 53  # integers below this (in magnitude) are exact in f64, and so is every sum / product / FMA of them


def int_conv(x, y, zshape):
    """z[k] = sum_{i + j = k} x[i] * y[j] for k inside `zshape`, in int64.  `x`, `y`: integer-valued arrays of one rank
    (f64 or int), every |partial sum| < 2^63 by the caller's bound.  One shifted slice multiply-add per non-zero
    coefficient of the smaller operand: no summation-order question, no floating point."""
    x, y = np.asarray(x), np.asarray(y)
    assert x.ndim == y.ndim == len(zshape)
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    assert np.array_equal(xi, x) and np.array_equal(yi, y), "operands must hold integers"
    if np.count_nonzero(xi) > np.count_nonzero(yi):
        xi, yi = yi, xi
    z = np.zeros(zshape, dtype=np.int64)
    for idx in zip(*np.nonzero(xi)):
        ext = tuple(min(zs - i, ys) for zs, i, ys in zip(zshape, idx, yi.shape))
        if min(ext) <= 0:
            continue
        dst = tuple(slice(i, i + e) for i, e in zip(idx, ext))
        src = tuple(slice(0, e) for e in ext)
        z[dst] += int(xi[idx]) * yi[src]
    return z


# ---- the product dispatcher's auto-mode decision (gft_ops_product.inc, K::conv), on shapes ---------------------------
TILED_MIN_MACS = 2.0e5            # Runtime::tiled_min_macs
RANK2_FACTOR, SPLIT_FACTOR = 4.0, 10.0
PAIRS_FIRST_MAX = {2: 2.0e8, 3: 1.0e7, 4: 1.0e6}  # pairs_first_max_rank2, pairs_first_max, 0.1 * pairs_first_max
PAIRS_MIN = {2: 1.0e6, 3: 3.0e5, 4: 3.0e5}        # rb_pairs_min_rank2, rb_pairs_min
SHALLOW_MAX_TERMS = 256


def conv_macs(xs, ys, zs):
    """(multiply-adds as the dispatcher estimates them, collapsed shapes) of the product xs (*) ys -> zs: unit axes of the
    result are dropped, every other axis counts 0.5 * zs * min(xs, ys)."""
    keep = [i for i, z in enumerate(zs) if z != 1]
    cx, cy, cz = ([int(s[i]) for i in keep] for s in (xs, ys, zs))
    macs = 1.0
    for a, b, c in zip(cx, cy, cz):
        macs *= 0.5 * c * min(a, b)
    return macs, cx, cy, cz


def product_path(xs, ys, zs):
    """Which kernel family the automatic dispatch gives a plain full f64 product of device tensors, from the shapes alone:
    'shallow', 'pairs' (the bit-exact row-pair form), 'tiled' (the 1e-10 contract) or 'reference'."""
    macs, cx, cy, cz = conv_macs(xs, ys, zs)
    nd = len(cz)
    if nd == 0:
        return "reference"
    terms = 1
    for a, b in zip(cx, cy):
        terms *= min(a, b)
    if terms <= SHALLOW_MAX_TERMS:
        return "shallow"
    if nd < 2:
        return "reference"
    if nd in PAIRS_FIRST_MAX and cy[-1] == cz[-1] and 8 <= cz[-1] <= 256 and PAIRS_MIN[nd] <= macs <= PAIRS_FIRST_MAX[nd] \
            and all(c <= a + b - 1 for a, b, c in zip(cx[:-1], cy[:-1], cz[:-1])):
        return "pairs"
    if nd > 4:
        if cz[-1] > 128:
            return "reference"
        lead = 1.0
        for a, b, c in zip(cx[:nd - 4], cy[:nd - 4], cz[:nd - 4]):
            lead *= 0.5 * c * min(a, b) + 0.5
        return "tiled" if macs / lead >= TILED_MIN_MACS else "reference"
    split = cz[-1] > 128
    if split and nd == 4:
        return "reference"
    factor = SPLIT_FACTOR if split else (RANK2_FACTOR if nd == 2 else 1.0)
    return "tiled" if macs >= TILED_MIN_MACS * factor else "reference"
