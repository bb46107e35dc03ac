"""The two transposed bivariate operations of genfer_amd.series2 (include/gftaylor.h: gft_series2_corr, gft_series2_compose_adj) in
plain Python, one IEEE operation at a time, written from their definitions.

``corr2(g, y, m)``: ``res[i0][i1] = 0.0 + sum_k0 (0.0 + sum_k1 g[k0][k1] * y[k0-i0][k1-i1])``, both sums DESCENDING over the stored
coefficients.  ``compose_adj(gh, g, var, nf)``: the transposed Horner loop over ``corr2`` at the compact shapes ``L_i`` of the forward
loop.  Every multiply and add is one numpy float64 scalar operation, so the order written here is the order of the roundings."""
import numpy as np

F = np.float64
ZERO = F(0.0)


def corr2(g, y, m):
    g, y = np.asarray(g, dtype=np.float64), np.asarray(y, dtype=np.float64)
    (g0, g1), (ny0, ny1), (m0, m1) = g.shape, y.shape, m
    assert ny0 <= g0 and ny1 <= g1 and m0 <= g0 and m1 <= g1
    res = np.empty((m0, m1), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i0 in range(m0):
            for i1 in range(m1):
                c = ZERO
                for k0 in range(min(g0 - 1, i0 + ny0 - 1), i0 - 1, -1):
                    o = ZERO
                    for k1 in range(min(g1 - 1, i1 + ny1 - 1), i1 - 1, -1):
                        o = o + g[k0, k1] * y[k0 - i0, k1 - i1]
                    c = c + o
                res[i0, i1] = c
    return res


def compact_shapes(nf, ng, n, var):
    """L_i, i < S: the stored shapes of the forward Horner loop, the last step first"""
    S, ln = (nf[0], nf[1]) if var == 0 else (nf[1], nf[0])
    base = (1, ln) if var == 0 else (ln, 1)
    return [tuple(min(base[a] + (S - 1 - i) * (ng[a] - 1), n[a]) for a in (0, 1)) for i in range(S)]


def compose_adj(gh, g, var, nf, corr=corr2):
    """``corr``: the product's adjoint at every step (the GPU tests pass series2.corr on tensors: the unfused loop)"""
    n, ng = tuple(gh.shape[-2:]), tuple(g.shape[-2:])
    L = compact_shapes(nf, ng, n, var)
    S, ln = len(L), (nf[1] if var == 0 else nf[0])
    a = gh[..., :L[0][0], :L[0][1]]
    slices = []
    for i in range(S):
        slices.append(a[..., 0, :ln] if var == 0 else a[..., :ln, 0])
        if i + 1 < S:
            a = corr(a, g, L[i + 1])
    if isinstance(gh, np.ndarray):
        return np.stack(slices, axis=-2 if var == 0 else -1)
    import torch

    return torch.stack(slices, dim=-2 if var == 0 else -1)
