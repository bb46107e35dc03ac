"""Data, references and case tables shared by test_streaming_variants_cpu.py and test_streaming_variants_gpu.py.

Every case names the dispatch condition it selects (file:line in genfer_amd/csrc) so that a reader sees which kernel it
is meant to reach.  The references here are plain numpy / math.fsum: none of them shares code with the oracle.
"""
import math

import numpy as np

from conftest import splitmix64_uniform

U = 2.0 ** -53  # unit roundoff of binary64


def numel(shape):
    return int(np.prod(shape)) if len(shape) else 1


# ---- three kinds of data ----------------------------------------------------------------------------------------------
def int_data(shape, seed):
    """Integers in [-1000, 1000]: at most 4097 of them are summed per output, so every partial sum in every order stays
    below 2^23 in magnitude — far below 2^53 — and every summation order is exact."""
    return np.floor(splitmix64_uniform(seed, numel(shape)) * 2001.0 - 1000.0).reshape(shape)


def pos_data(shape, seed):
    """Strictly positive: [0.5, 1.5)."""
    return (0.5 + splitmix64_uniform(seed, numel(shape))).reshape(shape)


def cancel_data(shape, seed):
    """Mixed signs over 40 binades; neighbours along the last axis cancel to ~2^-30 of their size (an unpaired last
    element is that small itself), so a row sum is many orders of magnitude below its terms."""
    n = numel(shape)
    u = splitmix64_uniform(seed, 3 * n).reshape((3,) + tuple(shape))
    x = (u[0] - 0.5) * np.exp2(np.floor(u[1] * 40.0))
    half = shape[-1] // 2
    x[..., 1 : 2 * half : 2] = -x[..., 0 : 2 * half : 2] * (1.0 + u[2][..., 1 : 2 * half : 2] * 2.0 ** -30)
    if shape[-1] % 2 and shape[-1] > 1:
        x[..., -1] *= 2.0 ** -30
    return x


DATA = {"int": int_data, "pos": pos_data, "cancel": cancel_data}


def as_interval(x, point=False):
    """[2, ...] = (lo, hi): point intervals, or x widened by 1e-9 relative."""
    if point:
        return np.stack([x, x])
    w = 1e-9 * np.abs(x)
    return np.stack([x - w, x + w])


# ---- references for shift_down(v, n)  (mt:514-536) -----------------------------------------------------------------------
def shift_down_exact(arr, v, n):
    """Exact result on integer-valued data, in int64: slab 0 is the sum of slabs 0..n, the rest moves down."""
    a = np.moveaxis(np.asarray(arr), v, 0)
    ai = a.astype(np.int64)
    assert np.array_equal(ai.astype(np.float64), a), "the data is not integer-valued"
    head = ai[: n + 1].sum(axis=0, keepdims=True)
    assert np.abs(ai[: n + 1]).sum(axis=0).max() < 2 ** 53
    return np.moveaxis(np.concatenate([head, ai[n + 1 :]], axis=0), 0, v)


def summed_terms(arr, v, n):
    """The terms that go into slab 0, as [m, outputs]."""
    t = np.moveaxis(np.asarray(arr), v, 0)[: n + 1]
    return t.reshape(t.shape[0], -1)


def assert_within_fsum_bound(arr, v, n, got, who):
    """|got - fsum(terms)| <= m u S / (1 - m u) per output of slab 0, with S = sum |terms| and m the number of additions
    into that output (one per term: the accumulator starts from zero; the first, 0 + x, is exact, which pays for the
    half-ulp of the correctly rounded reference).  The bound holds for ANY summation order (Higham, Accuracy and Stability
    of Numerical Algorithms, §4.2), so it is a property of the operation, not of a kernel.  The slabs behind slab 0 are
    copies and must be the input's bits."""
    t = summed_terms(arr, v, n)
    m = t.shape[0]
    assert t.shape[1] <= 20000, "fsum reference: keep the number of outputs small"
    g = np.moveaxis(np.asarray(got), v, 0)
    g0 = g[0].reshape(-1)
    cols = t.T.tolist()
    worst = 0.0
    for j, col in enumerate(cols):
        ref = math.fsum(col)
        S = math.fsum(abs(x) for x in col)
        bound = m * U * S / (1.0 - m * U)
        err = abs(g0[j] - ref)
        if bound > 0:
            worst = max(worst, err / bound)
        assert err <= bound, f"{who}: output {j}: got {g0[j]!r}, fsum {ref!r}, |err| {err:.3e} > bound {bound:.3e} (m={m}, S={S:.3e})"
    rest = np.moveaxis(np.asarray(arr), v, 0)[n + 1 :]
    assert np.array_equal(g[1:], rest), f"{who}: the slabs behind slab 0 are not copies of the input"
    return worst


# ---- shift_down cases -----------------------------------------------------------------------------------------------------
# (id, stored shape, degrees_p1, v, n, order): order "wave" = the butterfly kernel (REL_TOL against the oracle on positive
# data), "ref" = a reference-order kernel (bit for bit the oracle).  deg[v] > n always (mt:515), so n may be large.
WAVE_LENGTHS = (127, 128, 129, 191, 192, 193, 1000, 4097)
WAVE_ROWS = (1, 3, 4, 5)


def wave_cases(L):
    """Full sums of rows of length L (shape[v] <= n + 1: gft_ops_observe.inc:459, upto = shape[v])."""
    out = []
    for rows in WAVE_ROWS:
        n = L - 1 + 4 * (rows % 2)
        # gft_ops_observe.inc:448 — W == 1 && inner == 1 && upto >= 128 -> SUM_WAVE; L = 127 stays on SUM_UNROLL8 (:442)
        out.append((f"full-{rows}x{L}", (rows, L), (rows, n + 2), 1, n, "wave" if L >= 128 else "ref"))
    return out


WAVE_EXTRA = [
    # gft_kernels.hip:1641-1642 — 2048 blocks x 4 waves = 8192 rows per pass: row 8192 is a second trip of wave 0
    ("full-8193x129", (8193, 129), (8193, 129), 1, 128, "wave"),
    # ... and with row_stride (131) != len (128): the prefix sum of gft_ops_observe.inc:486 (upto = n)
    ("prefix-8193x131-n128", (8193, 131), (8193, 131), 1, 128, "wave"),
    # gft_ops_observe.inc:486 — prefix of a longer row: len = 200, row_stride = 300
    ("prefix-5x300-n200", (5, 300), (5, 300), 1, 200, "wave"),
    # upto = n = 128: the first prefix length that takes the wave kernel; 127 does not (SUM_UNROLL8 with stride 500)
    ("prefix-3x500-n128", (3, 500), (3, 500), 1, 128, "wave"),
    ("prefix-3x500-n127", (3, 500), (3, 500), 1, 127, "ref"),
    # lane loop k += 64 (gft_kernels.hip:1607): 1000 = 15 full trips + 40 lanes
    ("prefix-4x1200-n1000", (4, 1200), (4, 2000), 1, 1000, "wave"),
    # rank 3, rows = product of the leading axes (gft_ops_observe.inc:437-439)
    ("rank3-full-3x4x193", (3, 4, 193), (3, 4, 193), 2, 192, "wave"),
    ("rank3-prefix-2x3x300-n200", (2, 3, 300), (2, 3, 301), 2, 200, "wave"),
    # rank 3, upto = 127 < 128: k_sum_axis_seq in SUM_SEQ with inner == 1 (gft_kernels.hip:1653; rank != 2 so no fold)
    ("rank3-prefix-2x3x300-n127", (2, 3, 300), (2, 3, 300), 2, 127, "ref"),
]

UNROLL8_LENGTHS = (7, 8, 9, 15, 16, 17, 64, 100)


def unroll8_cases(L):
    """Rank 2 with a unit-stride summed axis: the 8-accumulator fold (gft_ops_observe.inc:442, gft_kernels.hip:1573-1586;
    host tier gft_host.hpp:300).  L < 8: tail loop only; 8 | L: no tail; otherwise both."""
    return [
        (f"fold-full-5x{L}", (5, L), (5, L), 1, L - 1, "ref"),
        (f"fold-prefix-5x{L + 3}-n{L}", (5, L + 3), (5, L + 3), 1, L, "ref"),  # len = L, lane stride L + 3
        (f"fold-axis0-{L}x1", (L, 1), (L, 1), 0, L - 1, "ref"),  # v = 0 with shape[1] == 1: inner == 1 too
        (f"fold-axis0-prefix-{L + 2}x1-n{L}", (L + 2, 1), (L + 2, 4), 0, L, "ref"),
    ]


def seq_cases():
    """Middle and leading axes: k_sum_axis_seq (odd inner) / k_sum_axis_seq_f64x2 (even inner, gft_kernels.hip:1647),
    prefix (n < shape[v] - 1) and full sums, n = 1, 8, 200."""
    out = []
    for v in (0, 1):
        for last in (6, 7):  # inner = 3 * last (v = 0) or last (v = 1): even -> f64x2, odd -> seq
            for n, Lv in ((1, 5), (1, 2), (8, 12), (8, 9), (200, 203), (200, 150)):
                shape = (Lv, 3, last) if v == 0 else (3, Lv, last)
                deg = tuple(max(s, n + 1) for s in shape)
                out.append((f"seq-v{v}-{'x'.join(map(str, shape))}-n{n}", shape, deg, v, n, "ref"))
    for n, Lv in ((1, 4), (8, 9), (200, 230)):  # rank 2, leading axis, inner > 1: SUM_SEQ, not the fold
        for last in (4, 5):
            out.append((f"seq-rank2-{Lv}x{last}-n{n}", (Lv, last), (max(Lv, n + 1), last), 0, n, "ref"))
    # compact tensor (stored 5 < degree 9 along v) with axis_stride_outer = 5 * 7 odd: gft_kernels.hip:1647 needs it even.
    # (With inner even, shape[v] * inner is even too: the odd-stride side is always k_sum_axis_seq.)
    out.append(("seq-compact-3x5x7-n2", (3, 5, 7), (3, 9, 7), 1, 2, "ref"))
    out.append(("seq-compact-3x5x7-n6", (3, 5, 7), (3, 9, 7), 1, 6, "ref"))
    out.append(("seq-compact-3x5x8-n2", (3, 5, 8), (3, 9, 8), 1, 2, "ref"))  # its f64x2 twin
    return out


# More outputs than one grid pass (grid_for caps at 2048 x 256 = 524 288 threads).  Integer and positive data only: an
# fsum per output would take seconds here, and the kernels' per-output order is pinned by the small cases.
BIG_SEQ_CASES = [
    # 3 x 200001 = 600 003 outputs, odd inner: k_sum_axis_seq's grid-stride second trip (gft_kernels.hip:1567)
    ("big-seq-3x3x200001-v1", (3, 3, 200001), (3, 3, 200001), 1, 2, "ref"),
    ("big-seq-3x3x200001-v0-prefix", (3, 3, 200001), (3, 3, 200001), 0, 1, "ref"),
    # 3 x 200001 = 600 003 PAIRS, even inner: k_sum_axis_seq_f64x2's second trip (gft_kernels.hip:1619)
    ("big-x2-3x3x400002-v1", (3, 3, 400002), (3, 3, 400002), 1, 2, "ref"),
    ("big-x2-3x3x400002-v0-prefix", (3, 3, 400002), (3, 3, 400002), 0, 1, "ref"),
]
# intervals always take k_sum_axis_seq<EInterval> (gft_kernels.hip:1647 is W == 1 only): 524 291 outputs, 8 MB a plane
BIG_INTERVAL_CASE = ("big-interval-2x524291-v0", (2, 524291), (2, 524291), 0, 1, "ref")


def small_shift_cases():
    out = []
    for L in WAVE_LENGTHS:
        out += wave_cases(L)
    out += [c for c in WAVE_EXTRA if numel(c[1]) <= 1 << 16]
    for L in UNROLL8_LENGTHS:
        out += unroll8_cases(L)
    return out + seq_cases()


# ---- verdict scans ------------------------------------------------------------------------------------------------------------
# k_linear_scan (gft_kernels.hip:1067): B = 128 blocks, or 1024 above 2^22 elements (:1148); per trip a thread looks at
# lin, lin + step, lin + 2 step, lin + 3 step (clamped to total - 1), step = 256 B; then lin += 4 step.
SCAN_SHAPES = [
    ((50, 64, 65), 128),    # 208 000 elements: 128 blocks, step 32 768, second trip from 131 072
    ((65, 254, 255), 1024),  # 4 210 050 > 2^22: 1024 blocks, step 262 144, second trip from 1 048 576
]


def spoiler_positions(shape, blocks):
    total, step = numel(shape), 256 * blocks
    assert 4 * step < total - 1
    # 1 = unit position of the LAST axis (a second variable), 2 = index 2 of it; first / last thread of the second, third
    # and fourth clamped loads; last element of the first trip, first of the second; the last element of the tensor
    return [1, 2, step - 1, step, 2 * step + 5, 3 * step + 5, 4 * step - 1, 4 * step, total - 1]


def linear_tensor(shape, c=0.75, m=-1.5):
    """c + m * x_0 in a full-size tensor: linear in axis 0 (mt:275-294)."""
    t = np.zeros(shape)
    t.flat[0] = c
    t[(1,) + (0,) * (len(shape) - 1)] = m
    return t


EQ_SHAPE = (1025, 1025)  # 1 050 625 elements: k_count_neq's grid stride takes a third trip (gft_kernels.hip:1664)
EQ_POSITIONS = [0, 524288 + 5, 2 * 524288 + 5, 1025 * 1025 - 1]
