"""Data that leaves the fast paths of the division / log / exp kernels (gft_div2d.hip) in the MIDDLE of a computation, and
the table of the smallest shapes that reach each of those kernels on the device tier.

The kernels switch at run time between a fast form and a slower one in three places:
  * the three-instruction quotient, valid while both exponents pass `fd_mid` (biased 724 .. 1322, i.e. 2^-299 .. 2^299);
  * the dropped bounds (excluded positions multiply a staged zero), exact while every quotient coefficient is finite;
  * the sign of an exact-zero coefficient ("a partial sum formed from +0 is never -0").
The families below make the RECURRENCE ITSELF carry a value across a switch — at coefficient 150 of a row, at slab 17 of a
quotient — instead of planting a special value in the input's first coefficients:

  growth(shape, axis)  the divisor holds (1 - t)(1 - g t) along `axis` (and +-1e-3 elsewhere): the quotient grows like g^k,
                       leaves the window upwards, overflows to one inf and continues as NaN;
  decay(shape)         dividend and divisor scaled by 2^(-b * sum of indices): the quotient is the unscaled one times the
                       same factor — normal values below the window, denormals, +0 and -0;
  divisor_sweep(n)     a divisor whose first and last stored entries alone are non-zero: coefficients 0 .. n - 2 of the
                       quotient are the INDEPENDENT quotients x[c] / d, so that one division checks n - 1 numerators against
                       numpy's correctly rounded x / d.

Every growth / decay case also exists with a compact divisor (about a quarter of the result along every axis, at least 3
entries) and with a compact dividend (half): a compact operand is what makes the dropped bounds matter — inf * (staged zero)
is NaN where the reference never forms the product.

Where a growth variant exists.  The probes (tests/test_recur_edges_cpu.py) ask that the first coefficient outside the window
has index >= 8 on the growth axis and that an inf and a NaN follow inside the extent.  The coefficients grow like 2^(b k):
leaving the window at k >= 8 needs 8 b < 300, the overflow (2^1024) then comes at k > 1024 / 37.5 = 27.3 and the first NaN
one or two steps later.  An axis shorter than GROWTH_MIN_EXTENT = 32 therefore cannot carry a growth variant; such shapes
((70, 24) along its rows, (4, 4, 5, 20), (2048, 8) along its rows, ...) get the axis-0 variant where that axis is long
enough, and always the decay family, which needs nothing of any single axis.

Out of scope: a NaN whose payload is the wavefront kernels' EMPTY pattern (DWF_EMPTY / RING_EMPTY in gft_div2d.hip, "a
genuine coefficient of that pattern only costs time").  That path fails by waiting, not by wrong bits; no generator here
produces such a NaN (all NaNs below come out of inf - inf / inf * 0 in the kernels themselves).

All comparisons are on uint64 bit patterns; a NaN only has to be a NaN (`same_bits`).
"""
import numpy as np

from conftest import splitmix64_uniform

INTERVAL_MAX_COEFFS = 20000  # the interval oracle's cost limit (~80 instructions a multiply-add), as in test_parity_gpu.py
GROWTH_MIN_EXTENT = 32       # see the module docstring
WIN_LO, WIN_HI = 724, 1322   # fd_mid: biased exponents inside the window


def rand(shape, seed, lo=0.0, hi=1.0):
    n = int(np.prod(shape)) if len(shape) else 1
    return (lo + (hi - lo) * splitmix64_uniform(seed, n)).reshape(shape)


# ---- classification of results (the probes and the failure messages) ---------------------------------------------------------


def biased_exponent(a):
    return ((np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)


def classify(a):
    """boolean masks over `a`: in the window, finite above it, normal below it, denormal, +0, -0, inf, NaN"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    e = biased_exponent(a)
    neg = np.signbit(a)
    return {
        "in_window": (e >= WIN_LO) & (e <= WIN_HI),
        "above": (e > WIN_HI) & (e < 0x7FF),
        "below": (e >= 1) & (e < WIN_LO),
        "denormal": (e == 0) & (a != 0.0),
        "pos_zero": (a == 0.0) & ~neg,
        "neg_zero": (a == 0.0) & neg,
        "inf": np.isinf(a),
        "nan": np.isnan(a),
    }


def same_bits(want, got):
    """mask of the coefficients that agree: the same 64 bits, or a NaN where the expected value is a NaN"""
    want, got = np.ascontiguousarray(want, dtype=np.float64), np.ascontiguousarray(got, dtype=np.float64)
    return (want.view(np.uint64) == got.view(np.uint64)) | (np.isnan(want) & np.isnan(got))


def describe_mismatch(what, want, got):
    """None if all bits agree, else a message with the first three differing indices and both values"""
    if want.shape != got.shape:
        return f"{what}: stored shape {got.shape} != {want.shape}"
    ok = same_bits(want, got)
    if ok.all():
        return None
    idx = np.argwhere(~ok)
    first = "; ".join(f"{tuple(int(v) for v in i)}: got {got[tuple(i)]!r} ({int(got[tuple(i)].view(np.uint64)):#018x}) "
                      f"want {want[tuple(i)]!r} ({int(want[tuple(i)].view(np.uint64)):#018x})" for i in idx[:3])
    return f"{what}: {len(idx)} of {want.size} coefficients differ, first at {first}"


# ---- the families ----------------------------------------------------------------------------------------------------------------

# exponent b of the growth factor g = 2^b per extent of the growth axis: leaves the window at 15 - 25 % of the extent, overflows
# at 60 - 80 % (checked on the oracle by test_recur_edges_cpu.py; other extents: 1400 / extent, the same proportions)
GROWTH_B = {32: 36.0, 64: 20.0, 256: 5.0, 512: 2.5, 1024: 1.6, 4096: 0.4}
# exponent b of the decay per shape (others: 1200 / (sum of the largest indices): zeros in the last tenth of the index sums)
DECAY_B = {(64,): 20.0, (256,): 5.0, (1024,): 1.3, (4096,): 0.3, (70, 48): 12.0, (24, 130): 9.0, (6, 7, 70): 16.0}


def growth_b(extent):
    return GROWTH_B.get(extent, 1400.0 / extent)


def decay_b(shape):
    shape = tuple(shape)
    return DECAY_B.get(shape, 1200.0 / max(1, sum(s - 1 for s in shape)))


def compact_divisor_shape(shape):
    return tuple(min(s, max(3, (s + 3) // 4)) for s in shape)


def compact_dividend_shape(shape):
    return tuple(min(s, max(3, (s + 1) // 2)) for s in shape)


def decay_dividend_shape(shape):
    """The decay family's compact dividend: three quarters along axis 0 and along the last axis.  Beyond the dividend's box a
    numerator is -(partial sum), and a partial sum that is zero is +0: every exact-zero quotient there is -0 / y0, one sign
    only.  Zeros of BOTH signs need underflow inside the box, so the box is larger than the growth family's half and the
    exponent is raised until the zeros begin inside it (decay_b_for_box)."""
    last = len(shape) - 1
    return tuple(min(s, max(3, (3 * s + 3) // 4)) if a in (0, last) else s for a, s in enumerate(shape))


def decay_b_for_box(shape, box):
    """zeros (below 2^-1075) from 85 % of the box's largest index sum on, but 2^(-7 b) still inside the window"""
    reach = max(1, sum(s - 1 for s in box))
    return min(41.0, max(decay_b(shape), 1100.0 / (0.85 * reach)))


def growth(shape, axis, xs=None, ys=None, b=None, seed=2201):
    """(x, y): x uniform in +-1 with x[0..0] = 1; y[0..0] = 1, y[e_axis] = -(1 + g), y[2 e_axis] = g, the rest uniform in +-1e-3.
    xs / ys: compact operand shapes (default: `shape`)."""
    shape = tuple(shape)
    xs, ys = tuple(xs or shape), tuple(ys or shape)
    assert ys[axis] >= 3
    g = float(np.exp2(growth_b(shape[axis]) if b is None else b))
    x = rand(xs, seed, -1.0, 1.0)
    x[(0,) * len(xs)] = 1.0
    y = rand(ys, seed + 1, -1e-3, 1e-3)
    e = [0] * len(ys)
    y[tuple(e)] = 1.0
    e[axis] = 1
    y[tuple(e)] = -(1.0 + g)
    e[axis] = 2
    y[tuple(e)] = g
    return x, y


def _index_sum(shape):
    s = np.zeros(shape)
    for ax, n in enumerate(shape):
        s = s + np.arange(n, dtype=np.float64).reshape([n if a == ax else 1 for a in range(len(shape))])
    return s


def decay(shape, xs=None, ys=None, b=None, seed=2301, y0=1.5):
    """(x, y): x = +-U(0.5, 1) * 2^(-b * sum of indices), y = U(-0.05, 0.05) * 2^(-b * sum of indices), y[0..0] = y0."""
    shape = tuple(shape)
    xs, ys = tuple(xs or shape), tuple(ys or shape)
    b = decay_b(shape) if b is None else b
    mag = 0.5 + 0.5 * rand(xs, seed)
    sign = np.where(rand(xs, seed + 1) < 0.5, -1.0, 1.0)
    x = sign * mag * np.exp2(-b * _index_sum(xs))
    y = rand(ys, seed + 2, -0.05, 0.05) * np.exp2(-b * _index_sum(ys))
    y[(0,) * len(ys)] = y0
    return x, y


# ---- the divisor sweep -----------------------------------------------------------------------------------------------------------

EDGE_EXPONENTS = (-300, -299, 299, 300)  # the two sides of each edge of fd_mid (values 2^e * [1, 2))


def _mantissas(seed, n):
    """n values in [1, 2) with random 52-bit mantissas"""
    m = (splitmix64_uniform(seed, n) * 4503599627370496.0).astype(np.uint64)  # 2^52
    return (m | np.uint64(0x3FF0000000000000)).view(np.float64)


def sweep_divisors(reduced=False):
    """at least 64 random 52-bit mantissas of both signs, 1 + ulp and 2 - ulp, each also at the four edge exponents.
    reduced (shapes whose oracle division takes a second): five divisors, one per exponent — a random negative mantissa inside
    the window, 2 - ulp and 1 + ulp on the two sides of its lower edge, random mantissas on the two sides of its upper edge; the
    numerators of each still cover the whole double range."""
    if reduced:
        m = _mantissas(2401, 3)
        return np.array([-m[0], np.ldexp(np.nextafter(2.0, 1.0), -300), np.ldexp(np.nextafter(1.0, 2.0), -299),
                         np.ldexp(m[1], 299), np.ldexp(-m[2], 300)])
    base = _mantissas(2401, 64)
    base = base * np.where(np.arange(base.size) % 2 == 0, 1.0, -1.0)
    base = np.concatenate([base, [np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0)]])
    return np.concatenate([base] + [np.ldexp(base, e) for e in EDGE_EXPONENTS])


def sweep_numerators(d, count, seed):
    """`count` numerators for the divisor d, every quotient finite (an inf would reach the following coefficients through
    q * 0): random mantissas at exponents spread over the whole double range — the four edge exponents among them — and the
    triples fl(d * m), the value below it and the value above it for random m."""
    ed = int(np.floor(np.log2(abs(d))))
    n_spread = count // 2
    spread = np.linspace(-1070, 1023, max(n_spread - 8, 1)).astype(np.int64)
    exps = np.concatenate([spread, np.repeat(np.array(EDGE_EXPONENTS, dtype=np.int64), 2)])[:n_spread]
    exps = np.minimum(exps, ed + 1020)  # |x / d| < 2^1022
    m = _mantissas(seed, n_spread) * np.where(splitmix64_uniform(seed + 1, n_spread) < 0.5, -1.0, 1.0)
    out = [np.ldexp(m, exps.astype(np.int32))]
    n_tri = count - n_spread
    mm = _mantissas(seed + 2, (n_tri + 2) // 3)
    # quotient exponents spread over -40 .. 40, pulled inside the double range around d
    qe = np.clip(np.linspace(-40, 40, mm.size).astype(np.int64), -1000 - ed, 1000 - ed)
    mm = np.ldexp(mm, qe.astype(np.int32)) * np.where(np.arange(mm.size) % 3 == 0, -1.0, 1.0)
    p = d * mm
    tri = np.stack([p, np.nextafter(p, -np.inf), np.nextafter(p, np.inf)], axis=1).reshape(-1)[:n_tri]
    out.append(tri)
    x = np.concatenate(out)
    assert x.size == count and np.all(np.isfinite(x / d))
    return x


def divisor_sweep(shape, d, seed=2501):
    """(x, y, valid): y has only its first and last stored entries non-zero (y[0..0] = d), x holds numerators; `valid` marks the
    coefficients of the quotient that equal x / d — all but those that the last entry of y reaches (the last one only)."""
    shape = tuple(shape)
    n = int(np.prod(shape))
    y = np.zeros(shape)
    y.flat[0] = d
    y.flat[n - 1] = 0.5
    x = np.zeros(n)
    x[:n - 1] = sweep_numerators(d, n - 1, seed)
    x[n - 1] = 1.0
    valid = np.ones(n, dtype=bool)
    valid[n - 1] = False
    return x.reshape(shape), y, valid.reshape(shape)


def negative_zero_rows(shape=(4, 8), x_rows=2):
    """(x, y): a dividend that ends after `x_rows` rows and a divisor with only its first and last entries non-zero: the rows
    beyond the dividend have partial sums of exactly +0, hence numerators -(+0) = -0 in EVERY coefficient, and the quotient
    there is -0 / 1.5 = -0.  The regression case of k_div_2d_rows64's speculative quotient, which answered +0 for such a row
    (no numerator of the row was outside the window, so nothing sent it to the full division)."""
    x = 1.0 + rand((x_rows, shape[1]), 2701)
    y = np.zeros(shape)
    y.flat[0] = 1.5
    y.flat[-1] = 0.5
    return x, y


# ---- the shape table -------------------------------------------------------------------------------------------------------------
# (kernel label, result shape, options, explicit compact shapes or None).  `family`: what plan_wavefront must answer for a
# division of the full shape with the wavefront on (None: not a wavefront shape); checked by test_recur_edges_cpu.py against
# tests/wavefront_plan_check.cpp.  `wf0`: the shape also runs with `div_wavefront` 0 (and the two results must agree).


class Row:
    def __init__(self, kernel, shape, family=None, wf0=False, cy=None, cx=None, cx_decay=None, log=False, exp=False, one_launch=False, intervals=True):
        self.kernel, self.shape, self.family = kernel, tuple(shape), family
        self.wf0 = wf0
        self.cy = tuple(cy) if cy else compact_divisor_shape(shape)
        self.cx = tuple(cx) if cx else compact_dividend_shape(shape)
        self.cx_decay = tuple(cx_decay) if cx_decay else (tuple(cx) if cx else decay_dividend_shape(shape))
        self.log, self.exp, self.one_launch, self.intervals = log, exp, one_launch, intervals

    @property
    def id(self):
        return "x".join(str(s) for s in self.shape)


TABLE = [
    # k_div_1d_wave<4 / 8 / 16>: one wave, 4 / 8 / 16 coefficients a lane
    Row("k_div_1d_wave<4>", (64,)), Row("k_div_1d_wave<4>", (256,)), Row("k_div_1d_wave<8>", (257,)),
    Row("k_div_1d_wave<8>", (512,)), Row("k_div_1d_wave<16>", (513,)), Row("k_div_1d_wave<16>", (1024,)),
    Row("k_div_1d_wave<16>", (600,), cy=(70,), cx=(300,)),
    # k_div_1d (LDS and a barrier a step) up to 4096, the serial kernel beyond
    Row("k_div_1d", (1025,)), Row("k_div_1d", (4096,)),
    # (one lane, 8.4e6 dependent steps: an interval division takes seconds on the device.  The kernel is one loop over E::div with
    # true bounds for both element types, without a fast path of its own: intervals only as the wide kind on the compact-divisor
    # variants, whose sums are a quarter as long)
    Row("k_div_1d_serial", (4097,), intervals="serial"),
    # the slab kernels (fewer than 64 rows: no wavefront)
    Row("k_div_2d_rows64", (20, 48), cy=(5, 20), log=True, exp=True), Row("k_div_2d_rows64", (63, 64), log=True),
    Row("k_div_2d", (6, 200)),
    # row by row, every row one fused k_div_1d launch
    Row("fused div_1d rows", (7, 700)),
    Row("fused div_1d rows", (40, 300), family="rows_2d", wf0=True, one_launch=True),
    Row("fused div_1d rows", (100, 200), family="rows_2d", wf0=True, one_launch=True),
    # k_div_wavefront, packed (rows <= 32) and not
    Row("k_div_wavefront", (70, 24), family="row", wf0=True, log=True, exp=True),
    Row("k_div_wavefront", (70, 48), family="row", wf0=True, log=True, exp=True),
    Row("k_div_wavefront", (9, 8, 33), family="row", wf0=True, log=True),
    Row("k_div_wavefront", (4, 4, 5, 20), family="row", wf0=True, log=True, cx_decay=(3, 4, 5, 20)),
    Row("k_div_wavefront_q<.,8>", (2048, 8), family="row_q8"),
    Row("k_div_wavefront_q<.,16>", (32, 64, 33), family="row_q16"),
    Row("k_rows_wavefront", (8, 65), family="rows_2d", log=True, exp=True, one_launch=True),
    Row("k_rows_wavefront", (24, 130), family="rows_2d", log=True, exp=True, one_launch=True),
    Row("k_seg_wavefront", (2, 4, 65), family="seg", log=True, one_launch=True),
    Row("k_seg_wavefront", (6, 7, 70), family="seg", log=True, one_launch=True),
    Row("k_seg_wavefront", (2, 2, 2, 66), family="seg", log=True, one_launch=True),
    # log's fused slab step (k_div_2d_rows64 with the dividend -acc + k * xs[k] and the stores q / k, (q / k) * k) needs a 2-d
    # SLAB: slabs of (6, 48) in a rank-3 argument, reached with `div_wavefront` 0 (with it on: k_div_wavefront's log mode).  Its
    # division takes the blocked recurrence either way (18 rows): k_div_2d_rows64 with the fused dividend -acc + xs[k].
    # (6, 48) itself: the rank-2 logarithm below the wavefront's 8 rows, whose slab divisions are single rows.
    Row("log fused slab step", (3, 6, 48), wf0=True, log=True),
    Row("log, rows as slabs", (6, 48), log=True),
]
ROWS = {r.id: r for r in TABLE}
assert len(ROWS) == len(TABLE)

# shapes whose quotient is checked coefficient by coefficient against x / d, one per kernel with a slab division of its own.
# (True: the reduced divisor list, for a shape whose oracle division takes up to a second: k_div_1d at its largest row, the
# fused rows, and k_div_wavefront_q<., 8> — the <., 16> instance is the same template and its smallest shape, (32, 64, 33), costs
# three seconds of oracle time a divisor: it is left to its decay cases.)
SWEEP_SHAPES = [((200,), False), ((600,), False), ((1100,), False), ((20, 48), False), ((6, 200), False), ((70, 48), False),
                ((8, 65), False), ((2, 4, 65), False), ((4096,), True), ((7, 700), True), ((2048, 8), True)]


def variants(row):
    """[(family name, axis or None, variant name, xs, ys)] of a table row"""
    out = []
    shape = row.shape
    fams = []
    axes = [len(shape) - 1] + ([0] if len(shape) > 1 else [])
    for ax in axes:
        if shape[ax] >= GROWTH_MIN_EXTENT:
            fams.append(("growth", ax))
    fams.append(("decay", None))
    for fam, ax in fams:
        out.append((fam, ax, "full", shape, shape))
        cy = row.cy
        if fam == "growth" and cy[ax] < 3:
            cy = tuple(3 if a == ax else s for a, s in enumerate(cy))
        out.append((fam, ax, "compact_divisor", shape, cy))
        out.append((fam, ax, "compact_dividend", row.cx if fam == "growth" else row.cx_decay, shape))
    return out


def case_id(row, fam, ax, var):
    return f"{row.id}-{fam}{'' if ax is None else ax}-{var}"


CASES = [(row, fam, ax, var, xs, ys) for row in TABLE for fam, ax, var, xs, ys in variants(row)]
CASE_IDS = [case_id(row, fam, ax, var) for row, fam, ax, var, _, _ in CASES]


def operands(row, fam, ax, xs, ys):
    if fam == "growth":
        return growth(row.shape, ax, xs, ys)
    return decay(row.shape, xs, ys, b=decay_b_for_box(row.shape, xs) if tuple(xs) != row.shape else None)


def interval_kinds(row, var=None):
    """[(name, widen)] — point intervals and [a, a + |a| * 1e-9] — for the shapes the interval oracle can afford"""
    if int(np.prod(row.shape)) > INTERVAL_MAX_COEFFS:
        return []
    kinds = [("point", lambda a: np.stack([a, a])), ("wide", lambda a: np.stack([a, a + np.abs(a) * 1e-9]))]
    if row.intervals == "serial":  # (see the table)
        return kinds[1:] if var == "compact_divisor" else []
    return kinds


LOG_CONSTANTS = (0.75, 1.5, 3.1)


def log_arguments(row):
    """[(name, argument)]: the decay divisor with three constant terms, and the growth divisor (1 - t)(1 - g t) along the last
    axis (times 1.5), whose logarithm ln 1.5 - sum (1 + g^k) / k t^k overflows like the quotient does"""
    out = [(f"decay_c{c}", decay(row.shape, y0=c)[1]) for c in LOG_CONSTANTS]
    if row.shape[-1] >= GROWTH_MIN_EXTENT:
        # (times 1.5: the constant term ln 1 = 0 would be a coefficient outside the window at index 0)
        out.append(("growth", 1.5 * growth(row.shape, len(row.shape) - 1)[1]))
    return out


# ---- expected values: computed once per process, shared by the CPU probes and the GPU comparisons --------------------------------

_cache = {}


def oracle_div(O, key, x, y, deg):
    k = (O.__qualname__, key)
    if k not in _cache:
        r = O.new(x, deg) / O.new(y, deg)
        a = np.asarray(r.array()).copy()
        a.setflags(write=False)
        _cache[k] = (a, r.degrees_p1(), r.coeffs_shape())
    return _cache[k]


def oracle_unary(O, key, op, x, deg):
    k = (O.__qualname__, op, key)
    if k not in _cache:
        r = getattr(O.new(x, deg), op)()
        a = np.asarray(r.array()).copy()
        a.setflags(write=False)
        _cache[k] = (a, r.degrees_p1(), r.coeffs_shape())
    return _cache[k]
