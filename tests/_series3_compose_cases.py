"""Expected values and cases shared by tests/test_series3_compose_cpu.py and tests/test_series3_compose_gpu.py.

The definition of genfer_amd.series3.compose / pow (include/gftaylor.h) three times over: the chains of general products built from
the oracle's orc_mul_raw at rank 3 (the expected value of the GPU tests), the same loops in plain Python on numpy float64 scalars,
one operation at a time (tests/_series3_model.py supplies the product), and the oracle's own subst_var / pow, which the chains
equal bit for bit wherever the oracle takes no shortcut.  Every product of a chain is series3.mul's -- its stored shape and its
squeeze of unit axes included; `unsqueezed_compose` runs the rank-3 loops in the caller's axis order instead (the tests' sentinel)."""
import numpy as np

import _series3_model as model
from _series3_oracle import dense, pad3, signed, want

POW_E = [0, 1, 2, 3, 5, 8, 13]


def mul3(oracle_lib, a, b, L):
    """series3.mul's definition on the stored shapes of a and b, truncated at L: orc_mul_raw at rank 3 on a zeroed result"""
    return want(oracle_lib, None, "mul", a[None], b[None], tuple(L))[0]


def compact(a, b, n):
    """the compact shape of a product of the stored shapes a and b under n (sum_shape)"""
    return tuple(min(a[i] + b[i] - 1, n[i]) for i in range(3))


def step_shapes(nf, ng, n, var):
    """the stored shapes of res through compose's loop, the start included"""
    r = tuple(1 if a == var else nf[a] for a in range(3))
    out = [r]
    for _ in range(nf[var] - 1):
        r = compact(r, ng, n)
        out.append(r)
    return out


def _horner(mul, f, g, var, n):
    """Horner over the slices of f along axis var, `mul(a, b, L)` the product"""
    f, g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
    cut = lambda i: tuple(slice(i, i + 1) if a == var else slice(None) for a in range(3))  # noqa: E731
    with np.errstate(all="ignore"):
        res = 0.0 + f[cut(f.shape[var] - 1)]
        for i in range(f.shape[var] - 2, -1, -1):
            res = np.array(mul(res, g, compact(res.shape, g.shape, n)))
            s = f[cut(i)]
            at = tuple(slice(0, s.shape[a]) for a in range(3))  # (index 0 on axis var: the slice has one coefficient there)
            res[at] = res[at] + s
    return pad3(res, n)


def _square_and_multiply(mul, x, e, n):
    with np.errstate(all="ignore"):
        res, base = np.array([[[1.0]]]), np.array(x, dtype=np.float64)
        while e > 0:
            if e & 1:
                res = mul(res, base, compact(res.shape, base.shape, n))
            e >>= 1
            if e > 0:
                base = mul(base, base, compact(base.shape, base.shape, n))
    return pad3(res, n)


def chain_compose(oracle_lib, f, g, var, n):
    return _horner(lambda a, b, L: mul3(oracle_lib, a, b, L), f, g, var, n)


def chain_pow(oracle_lib, x, e, n):
    return _square_and_multiply(lambda a, b, L: mul3(oracle_lib, a, b, L), x, e, n)


def model_compose(f, g, var, n):
    """the same loop with every product in plain Python (the slice add is one numpy float64 addition per coefficient)"""
    return _horner(model.mul, f, g, var, n)


def model_pow(x, e, n):
    return _square_and_multiply(model.mul, x, e, n)


def unsqueezed_compose(f, g, var, n):
    """the sentinel: every product by the rank-3 loops in the caller's axis order, one accumulator over (j0, j1) per row, whatever
    unit axes the step's shape has"""
    return _horner(lambda a, b, L: model._mul3(a, b, tuple(L)), f, g, var, n)


def want_compose(oracle_lib, F, G, var, n):
    """F: [B, nf0, nf1, nf2], G: [B, ng0, ng1, ng2] (or one item [ng0, ng1, ng2] for every b)"""
    return np.stack([chain_compose(oracle_lib, F[b], G[b] if G.ndim == 4 else G, var, n) for b in range(F.shape[0])])


def want_pow(oracle_lib, X, e, n):
    return np.stack([chain_pow(oracle_lib, X[b], e, n) for b in range(X.shape[0])])


def _stored(p, n):
    """what the oracle stores (fewer axes for a constant), extended with +0 to n"""
    a = np.asarray(p.array(), dtype=np.float64)
    return pad3(a.reshape(a.shape + (1,) * (3 - a.ndim)), n)


def oracle_compose(OTP, f, g, var, n):
    return _stored(OTP.new(f, n).subst_var(var, OTP.new(g, n)), n)


def oracle_pow(OTP, x, e, n):
    return _stored(OTP.new(x, n).pow(e), n)


# ---- the cases on which the oracle itself is the expected value (the CPU test re-establishes it) ------------------------------------

ORACLE_SHAPES = [(2, 2, 2), (3, 4, 5), (5, 3, 2), (4, 4, 8), (4, 4, 9), (8, 8, 8), (2, 2, 33), (1, 3, 4), (3, 1, 4), (3, 4, 1), (1, 1, 5), (4, 1, 1)]


def compact_shapes(n):
    """the stored shapes of a compact f (or x) and a compact g under a result of n"""
    return ((max(1, n[0] // 2), max(1, n[1] - 1), n[2]),
            (max(1, n[0] - 1), n[1], max(1, min(n[2], max(2, n[2] // 2)))))


def g_forms(n):
    """g of shape n, a compact g, min(2, n), and one unit axis at a time"""
    return [n, compact_shapes(n)[1], tuple(min(2, v) for v in n), (1, n[1], n[2]), (n[0], 1, n[2]), (n[0], n[1], 1)]


def two_slices(n, var):
    return tuple(min(2, n[a]) if a == var else n[a] for a in range(3))


def oracle_compose_cases(n):
    """(var, f shape, g shape, data): per var the six forms of g under a full f, a compact f and a two-slice f under a full g; each on
    dense and on signed data -- 48 per shape, repeats (at shapes with unit axes) included"""
    out = []
    for var in (0, 1, 2):
        pairs = [(n, gs) for gs in g_forms(n)] + [(compact_shapes(n)[0], n), (two_slices(n, var), n)]
        out += [(var, fs, gs, kind) for fs, gs in pairs for kind in ("dense", "signed")]
    return out


def oracle_pow_cases(n):
    """(x shape, data, e): a full x on dense and signed data, a compact x on dense data"""
    return [(xs, kind, e) for xs, kind in ((n, "dense"), (n, "signed"), (compact_shapes(n)[0], "dense")) for e in POW_E]


def make(kind, shape, seed):
    return (signed if kind == "signed" else dense)(shape, seed)


# the sentinels of the squeeze: (f shape, g shape, n, var)
SENTINELS = [((4, 3, 1), (3, 3, 1), (5, 4, 2), 0), ((3, 3, 4), (3, 3, 1), (4, 4, 4), 2)]
