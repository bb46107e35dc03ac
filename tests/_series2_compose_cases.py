"""Expected values and cases shared by tests/test_series2_compose_cpu.py and tests/test_series2_compose_gpu.py.

The definition of genfer_amd.series2.compose / pow (include/gftaylor.h) three times over: the chains of general products built from
the oracle's orc_mul_raw at rank 2 (the expected value of the GPU tests), the same loops in plain Python on numpy float64 scalars,
one operation at a time (tests/_series2_model.py supplies the product), and the oracle's own subst_var / pow, which the chains
equal bit for bit wherever the oracle takes no shortcut."""
import numpy as np

import _series2_model as model
from _series2_oracle import compact_shapes, dense, pad2, signed, want_mul

POW_E = [0, 1, 2, 3, 5, 8, 13]


def mul2(oracle_lib, a, b, L):
    """series2.mul's loop on the stored shapes of a and b, truncated at L: orc_mul_raw on a zeroed result"""
    return want_mul(oracle_lib, a[None], b[None], L)[0]


def _compact(a, b, n):
    return min(a.shape[0] + b.shape[0] - 1, n[0]), min(a.shape[1] + b.shape[1] - 1, n[1])


def _horner(mul, f, g, var, n):
    """Horner over the rows (var 0) or the columns (var 1) of f, `mul(a, b, L)` the product"""
    f, g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
    nf0, nf1 = f.shape
    with np.errstate(all="ignore"):
        if var == 0:
            res = 0.0 + f[nf0 - 1:nf0, :]
            for i in range(nf0 - 2, -1, -1):
                res = mul(res, g, _compact(res, g, n))
                res[0, :nf1] = res[0, :nf1] + f[i, :]
        else:
            res = 0.0 + f[:, nf1 - 1:nf1]
            for i in range(nf1 - 2, -1, -1):
                res = mul(res, g, _compact(res, g, n))
                res[:nf0, 0] = res[:nf0, 0] + f[:, i]
    return pad2(res, n)


def _square_and_multiply(mul, x, e, n):
    with np.errstate(all="ignore"):
        res, base = np.array([[1.0]]), np.array(x, dtype=np.float64)
        while e > 0:
            if e & 1:
                res = mul(res, base, _compact(res, base, n))
            e >>= 1
            if e > 0:
                base = mul(base, base, _compact(base, base, n))
    return pad2(res, n)


def chain_compose(oracle_lib, f, g, var, n):
    return _horner(lambda a, b, L: mul2(oracle_lib, a, b, L), f, g, var, n)


def chain_pow(oracle_lib, x, e, n):
    return _square_and_multiply(lambda a, b, L: mul2(oracle_lib, a, b, L), x, e, n)


def model_compose(f, g, var, n):
    """the same loop with every product in plain Python (the slice add is one numpy float64 addition per coefficient)"""
    return _horner(model.mul, f, g, var, n)


def model_pow(x, e, n):
    return _square_and_multiply(model.mul, x, e, n)


def want_compose(oracle_lib, F, G, var, n):
    """F: [B, nf0, nf1], G: [B, ng0, ng1] (or one item [ng0, ng1] for every b)"""
    return np.stack([chain_compose(oracle_lib, F[b], G[b] if G.ndim == 3 else G, var, n) for b in range(F.shape[0])])


def want_pow(oracle_lib, X, e, n):
    return np.stack([chain_pow(oracle_lib, X[b], e, n) for b in range(X.shape[0])])


def _stored(p, n):
    """what the oracle stores (fewer axes for a constant), extended with +0 to n"""
    a = np.asarray(p.array(), dtype=np.float64)
    return pad2(a.reshape(a.shape + (1,) * (2 - a.ndim)), n)


def oracle_compose(OTP, f, g, var, n):
    return _stored(OTP.new(f, n).subst_var(var, OTP.new(g, n)), n)


def oracle_pow(OTP, x, e, n):
    return _stored(OTP.new(x, n).pow(e), n)


# ---- the cases on which the oracle itself is the expected value (the CPU test re-establishes it) ------------------------------------

ORACLE_SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 4), (4, 8), (8, 8), (7, 9), (16, 16), (5, 33), (33, 5), (32, 32)]


def oracle_compose_cases(n):
    """(f shape, g shape, data) under a result of n: dense and compact pairs, g of stored shape (2, 2), (3, 3), (1, n1), (n0, 1), f
    with two slices; each on dense and on signed data.  Shapes the result does not admit are left out, repeats too."""
    fc, gc = compact_shapes(*n)
    pairs = [(n, n), (fc, gc), (n, (2, 2)), (n, (3, 3)), (n, (1, n[1])), (n, (n[0], 1))]
    seen = []
    for var in (0, 1):
        two = (min(2, n[0]), n[1]) if var == 0 else (n[0], min(2, n[1]))
        for fs, gs in pairs + [(two, n)]:
            if gs[0] > n[0] or gs[1] > n[1]:
                continue
            for kind in ("dense", "signed"):
                case = (var, fs, gs, kind)
                if case not in seen:
                    seen.append(case)
    return seen


def oracle_pow_cases(n):
    """(x shape, data, e): dense x on dense and signed data, compact x on dense data"""
    xc = compact_shapes(*n)[0]
    seen = []
    for xs, kind in ((n, "dense"), (n, "signed"), (xc, "dense")):
        for e in POW_E:
            if (xs, kind, e) not in seen:
                seen.append((xs, kind, e))
    return seen


def make(kind, shape, seed):
    return (signed if kind == "signed" else dense)(shape, seed)
