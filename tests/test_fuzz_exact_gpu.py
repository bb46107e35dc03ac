"""Seeded random expression trees on small-integer data ABOVE the tiled crossover: GPU vs the CPU oracle, value for value.

test_fuzz_gpu.py keeps its trees below the crossover, where every kernel has the reference's summation order.  Here the
products run on the kernels of the 1e-10 contract (tiled, peeled, inner split, high rank) through the handle API in auto
mode, with the lazy handles, memoised verdicts, deferred chains and pooled buffers of a real program around them — and
are still checked exactly: every leaf holds integers in [-3, 3] and the trees use ring operations only, so as long as
every partial sum stays below 2^53 each f64 operation is exact in ANY order, with or without FMA.  The generator proves
that bound as it goes (`Node.B`, an upper bound of the L1 norm of the coefficients: B(x +- y) = B(x) + B(y),
B(x * y) = B(x) B(y), B(c x) = |c| B(x), B(d/dx^n) <= (len - 1)..(len - n) B, Horner term by term) and retreats to a leaf
where an operation would reach 2^53.

Comparison: stored shape, degrees_p1 and the inspections (constant_term, extract_linear, is_zero) identical; the
coefficients with np.array_equal — VALUE equality, not bit patterns: the sign of an exact zero legitimately depends on the
summation order (an accumulator that starts at +0 and an FMA chain that starts from a -0 product end in different
zeros).  Nothing non-finite can occur, so any NaN is a failure.  The leaf-level products of every tree are also compared
with a plain int64 convolution (_exact_int.int_conv) that knows neither the oracle nor the library."""
import contextlib

import numpy as np
import pytest

from _exact_int import LIMIT, conv_macs, int_conv, product_path

# Oracle multiply-adds one parametrised case may spend on general products, all seeds together (the oracle runs ~1e9 of
# them a second; the int64 check of the leaf-level products costs about as much again).
CASE_MAC_BUDGET = 6.0e8
DEPTH = 3


def derivative_factors(n, count):
    """The factors (k + n)! / k!, k < count, as the reference forms them: a running product of f64 ratios (n + k + 1) /
    (k + 1).  They are integers mathematically, but that product rounds: from k = 26 on for n = 1 and k = 9 for n = 2 the
    f64 factor is no integer any more.  The generator differentiates only where every factor is one."""
    ff = 1.0
    for i in range(1, n + 1):
        ff *= float(i)
    out = []
    for k in range(count):
        out.append(ff)
        ff = ff * (float(n + k + 1) / float(k + 1))
    return out


class Node:
    """One tree node: a handle per backend, the proven L1 bound, and (dense leaves) the source array."""

    def __init__(self, h, B, arr=None):
        self.h, self.B, self.arr = h, B, arr


class ExactGen:
    """Gen of test_fuzz_gpu.py restated for integer data at a shape class: `Ts` are the backends (oracle first), every
    operation is applied to all of them in turn."""

    def __init__(self, seed, cls, Ts, mac_budget, check_nodes=False):
        self.rng = np.random.default_rng(seed)
        self.cls, self.Ts, self.deg = cls, Ts, list(cls["deg"])
        self.nv = len(self.deg)
        self.budget = mac_budget
        self.check_nodes = check_nodes
        self.products = []       # (path, macs) of every general product, by the dispatcher's own arithmetic
        self.leaf_products = []  # (x array, y array, node): products whose operands are dense leaves
        self.inspections = 0

    # -- plumbing
    def ap(self, f, B, *nodes, arr=None):
        assert B < LIMIT
        n = Node([f(T, *(m.h[i] for m in nodes)) for i, T in enumerate(self.Ts)], B, arr)
        if self.check_nodes:  # the bound against the actual tree (CPU test): max |coeff| <= B < 2^53 at every node
            a = np.asarray(n.h[0].array())
            assert np.all(np.isfinite(a)) and np.array_equal(a, np.rint(a)), "non-integer coefficient"
            assert (np.abs(a).max() if a.size else 0.0) <= B, (np.abs(a).max(), B)
        return n

    def inspect(self, n):
        """The interpreter's in-between reads, identical on every backend."""
        if self.rng.random() >= 0.35:
            return
        self.inspections += 1
        what = int(self.rng.integers(0, 3))
        vals = [(h.constant_term(), h.extract_linear(), h.is_zero())[what] for h in n.h]
        assert all(v == vals[0] for v in vals[1:]), (what, vals)

    # -- leaves
    def dense(self, shape, zero_prob=0.3):
        a = self.rng.integers(-3, 4, size=shape).astype(np.float64)
        if self.rng.random() < zero_prob:  # zero patterns: a zero leading slab, zero trailing rows, or nothing but zeros
            k = int(self.rng.integers(0, 3))
            if k == 0:
                a[0] = 0.0
            elif k == 1:
                a[..., shape[-1] // 2:] = 0.0
            elif self.rng.random() < 0.3:
                a[...] = 0.0
        deg = self.deg
        return self.ap(lambda T: T.new(a, deg), float(np.abs(a).sum()), arr=a)

    def class_leaf(self, zero_prob=0.3):
        """A dense leaf of one of the class's stored shapes."""
        shapes = self.cls["leaves"]
        shape = list(shapes[int(self.rng.integers(0, len(shapes)))])
        if self.cls.get("jitter") and self.rng.random() < 0.4:
            ax = int(self.rng.integers(0, self.nv))
            shape[ax] = max(1, shape[ax] - int(self.rng.integers(1, 4)))
        return self.dense(tuple(shape), zero_prob)

    def leaf(self):
        r = self.rng.random()
        deg, nv = self.deg, self.nv
        if r < 0.62:
            return self.class_leaf()
        if r < 0.72:  # a stencil: a compact operand that makes the product shallow
            return self.dense(tuple(int(self.rng.integers(1, min(3, d) + 1)) for d in deg), zero_prob=0.0)
        if r < 0.79:
            c = float(self.rng.integers(-3, 4))
            return self.ap(lambda T: T.from_scalar(c), abs(c))
        v = int(self.rng.integers(0, nv))
        if r < 0.86:
            n = int(self.rng.integers(2, deg[v] + 1))
            return self.ap(lambda T: T.var_at_zero(v, n), 1.0)
        x0 = float(self.rng.integers(-2, 3))
        if r < 0.93:
            n = int(self.rng.integers(1, deg[v] + 1))
            return self.ap(lambda T: T.var(v, x0, n), abs(x0) + 1.0)
        return self.ap(lambda T: T.var_with_degrees_p1(v, x0, deg), abs(x0) + 1.0)

    # -- products
    def note_product(self, x, y, z):
        xs, ys, zs = (tuple(n.h[0].coeffs_shape()) for n in (x, y, z))
        nd = max(len(xs), len(ys), len(zs))
        xs, ys, zs = (s + (1,) * (nd - len(s)) for s in (xs, ys, zs))
        macs = conv_macs(xs, ys, zs)[0]
        self.products.append((product_path(xs, ys, zs), macs))
        self.budget -= macs

    def product_macs(self, x, y):
        xs, ys = tuple(x.h[0].coeffs_shape()), tuple(y.h[0].coeffs_shape())
        dx, dy = x.h[0].degrees_p1(), y.h[0].degrees_p1()
        nd = max(len(xs), len(ys))
        xs, ys = xs + (1,) * (nd - len(xs)), ys + (1,) * (nd - len(ys))
        cap = [min(dx[i] if i < len(dx) else 2 ** 62, dy[i] if i < len(dy) else 2 ** 62) for i in range(nd)]
        zs = tuple(min(a + b - 1, c) for a, b, c in zip(xs, ys, cap))
        return conv_macs(xs, ys, zs)[0]

    def mul(self, x, y):
        if x.B * y.B >= LIMIT or self.product_macs(x, y) > self.budget:
            return self.leaf()
        z = self.ap(lambda T, a, b: a * b, x.B * y.B, x, y)
        self.note_product(x, y, z)
        if x.arr is not None and y.arr is not None:
            self.leaf_products.append((x.arr, y.arr, z))
        return z

    def power(self, x, e):
        if x.B ** e >= LIMIT or (e - 1) * self.product_macs(x, x) > self.budget:
            return self.leaf()
        z = self.ap(lambda T, a: a.pow(e), x.B ** e, x)
        self.note_product(x, x, z)
        if e == 3:
            self.note_product(z, x, z)
        if e == 2 and x.arr is not None:
            self.leaf_products.append((x.arr, x.arr, z))
        return z

    # -- trees
    def root(self, depth):
        """A random tree joined (* + -) to one product of two class leaves: whatever the random part retreats to, every
        tree holds a product of the class's shapes, and one whose operands the int64 convolution can check."""
        anchor = self.mul(self.class_leaf(0.1), self.class_leaf(0.1))
        t = self.tree(depth, top=True)
        r = self.rng.random()
        if r < 0.5 and t.B * anchor.B < LIMIT and self.product_macs(t, anchor) <= self.budget:
            n = self.mul(t, anchor) if r < 0.25 else self.mul(anchor, t)
        elif t.B + anchor.B < LIMIT:
            n = self.ap((lambda T, p, q: p + q) if r < 0.75 else (lambda T, p, q: q - p), t.B + anchor.B, t, anchor)
        else:
            n = anchor
        self.inspect(n)
        return n

    def tree(self, depth, top=False):
        if depth == 0 or (not top and self.rng.random() < 0.12):
            n = self.leaf()
            self.inspect(n)
            return n
        n = self.op(depth, top)
        self.inspect(n)
        return n

    def op(self, depth, top):
        r = self.rng.random()
        if top:  # the root is a product-bearing operation four times out of five
            r *= 0.5 if self.rng.random() < 0.8 else 1.0
        a = self.tree(depth - 1)
        if r < 0.34:
            return self.mul(a, self.tree(depth - 1))
        if r < 0.43:
            return self.power(a, 2)
        if r < 0.47:
            return self.power(a, 3)
        if r < 0.57:
            b = self.tree(depth - 1)
            if a.B + b.B >= LIMIT:
                return self.leaf()
            if self.rng.random() < 0.5:
                return self.ap(lambda T, p, q: p + q, a.B + b.B, a, b)
            return self.ap(lambda T, p, q: p - q, a.B + b.B, a, b)
        if r < 0.61:
            return self.ap(lambda T, p: -p, a.B, a)
        if r < 0.67:
            c = float(self.rng.integers(-3, 4))
            return self.ap(lambda T, p: p * T.from_scalar(c), abs(c) * a.B, a)
        nv = a.h[0].num_vars()
        if nv == 0:
            return a
        v = int(self.rng.integers(0, nv))
        ln = int(a.h[0].len_of(v))
        if r < 0.74:
            n = int(self.rng.integers(1, 3))
            stored = int(a.h[0].coeffs_shape()[v]) if v < len(a.h[0].coeffs_shape()) else 1
            factors = derivative_factors(n, max(stored - n, 1))
            factor = max(factors)
            if n >= ln or factor * a.B >= LIMIT or any(f != np.rint(f) for f in factors):
                return a
            return self.ap(lambda T, p: p.derivative(v, n), factor * a.B, a)
        if r < 0.79:
            if ln <= 1:
                return a
            return self.ap(lambda T, p: p.shift_down(v, 1), a.B, a)
        if r < 0.84:
            top_deg = max(self.deg)
            d = int(self.rng.integers(max(1, (2 * top_deg) // 3), top_deg + 1))
            return self.ap(lambda T, p: p.truncate_to_degree_p1(d), a.B, a)
        if r < 0.86 and nv < 5:
            d = int(self.rng.integers(1, 3))
            return self.ap(lambda T, p: p.extend_to_dim(nv + 1, d), a.B, a)
        if r < 0.89:
            k = int(self.rng.integers(0, min(ln, 3)))
            return self.ap(lambda T, p: p.coefficients_of_term(v, k), a.B, a)
        return self.subst(a, v, ln)

    def subst(self, a, v, ln):
        """subst_var with an integer series of zero constant term: c * x_w, or a small dense one (x_v + x_w-like)."""
        nv = a.h[0].num_vars()
        w = int(self.rng.integers(0, nv))
        if self.rng.random() < 0.6:
            c = float([1, -1, 2, -2][int(self.rng.integers(0, 4))])
            n = max(2, min(ln, self.deg[w] if w < self.nv else 2))
            s = self.ap(lambda T: T.var_at_zero(w, n) * T.from_scalar(c), abs(c))
        else:
            shape = [1] * nv
            deg = list(a.h[0].degrees_p1())
            shape[v], shape[w] = min(2, deg[v]), min(2, deg[w])
            arr = self.rng.integers(-1, 2, size=shape).astype(np.float64)
            arr.flat[0] = 0.0
            s = self.ap(lambda T: T.new(arr, deg), float(np.abs(arr).sum()))
        # Horner, term by term: every slice of `a` along v is bounded by a.B, slice k meets s^k
        B, pw = 0.0, 1.0
        for _ in range(ln):
            B += a.B * pw
            pw *= max(s.B, 1.0)
            if B >= LIMIT:
                return self.leaf()
        self.inspect(s)
        return self.ap(lambda T, p, q: p.subst_var(v, q), B, a, s)


# ---- shape classes: the smallest shapes at which the automatic dispatch reaches the named kernel ----------------------
# (deg = degree caps, leaves = stored shapes of the dense leaves; full x full products must exceed the row-pair form's
# pairs_first_* limit, 1e7 / 2e8 / 1e6 multiply-adds at rank 3 / 2 / 4, before the tiled kernel is asked at all — a y that is
# compact on the last axis is not the row-pair form's case, so there tiled_min_macs = 2e5 x 1 / 4 / 10 decides)
def _rank3(a, b, inner):
    return dict(deg=[a, b, inner], leaves=[(a, b, inner)], jitter=True)


CLASSES = {
    "rank3_inner8": _rank3(37, 35, 8),        # NW = 1, rows of one whole chunk
    "rank3_inner28": _rank3(21, 19, 28),      # packed rows (28 is no multiple of 8)
    "rank3_inner32": _rank3(19, 17, 32),      # NW = 2, whole-chunk rows
    "rank3_inner64": _rank3(13, 13, 64),      # NW = 4
    "rank3_inner128": _rank3(9, 9, 128),      # NW = 8, the longest unsplit last axis
    # operands that are results of earlier products: library buffers with slack, rows of whole chunks (32)
    "rank3_in_place": dict(deg=[23, 21, 32], leaves=[(12, 11, 16), (12, 11, 17)]),
    # full 16-multiple lane axes, tiled_peel = 1
    "rank3_peeled": dict(deg=[32, 16, 32], leaves=[(32, 16, 32)], options={b"tiled_peel": (1, -1)}, expect=("tiled_peeled",)),
    "rank2_direct": dict(deg=[90, 100], leaves=[(90, 93), (88, 96)]),              # 1 x 64 lane tile, no split
    "rank2_split_shortest": dict(deg=[61, 130], leaves=[(61, 125), (61, 121)]),    # rows just over the split's 128
    "rank2_split_ragged": dict(deg=[150, 200], leaves=[(100, 130), (70, 97)]),     # ragged, compact, pad / fold
    "rank2_split_long": dict(deg=[40, 264], leaves=[(40, 264)], jitter=True),      # beyond the row-pair form's 256
    "rank3_split129": dict(deg=[11, 9, 129], leaves=[(11, 9, 125), (11, 9, 120)]),
    "rank3_split300": dict(deg=[6, 5, 300], leaves=[(6, 5, 300), (5, 5, 290)]),
    "rank4": dict(deg=[5, 9, 9, 16], leaves=[(5, 9, 9, 16), (3, 9, 9, 16), (5, 6, 9, 13)]),  # uniform leading axis, compact outer axes
    "rank5_high_rank": dict(deg=[3, 4, 7, 7, 16], leaves=[(3, 4, 7, 7, 16), (2, 4, 7, 7, 16)]),
    # compact x full and full x compact, x's rows end inside a chunk (21); the caps cut axes 0 and 2, not axis 1 (22 + 17 - 1 = 38 < 40)
    "compact_full": dict(deg=[20, 40, 28], leaves=[(13, 22, 21), (20, 17, 28)], expect=("shallow_products",)),
}
SEEDS = 4


def _trees(name, Ts, check_nodes=False, seeds=SEEDS):
    """Yield (generator, root node) of every seeded tree of the class."""
    cls = CLASSES[name]
    salt = 7919 * (1 + sorted(CLASSES).index(name))
    for s in range(seeds):
        gen = ExactGen(salt + s, cls, Ts, CASE_MAC_BUDGET / seeds, check_nodes)
        yield gen, gen.root(DEPTH)


def _embed(a, shape):
    out = np.zeros(shape, dtype=a.dtype)
    out[tuple(slice(0, s) for s in a.shape)] = a
    return out


def _equal_as_series(a, b):
    """Value equality of two coefficient arrays of one rank as truncated series (a shorter axis means zeros beyond it)."""
    if a.ndim != b.ndim:
        return False
    shape = tuple(max(s, t) for s, t in zip(a.shape, b.shape))
    return np.array_equal(_embed(a, shape), _embed(b, shape))


def _check_leaf_products(gen, backend):
    """Every leaf-level product of the tree against the plain int64 convolution."""
    for x, y, z in gen.leaf_products:
        got = np.asarray(z.h[backend].array())
        assert not np.isnan(got).any()
        zs = tuple(min(a + b - 1, c) for a, b, c in zip(x.shape, y.shape, gen.deg))
        want = int_conv(x, y, zs)
        assert np.abs(want).max(initial=0) < LIMIT
        assert _equal_as_series(got, want.astype(np.float64)), (x.shape, y.shape, zs)


def test_int_conv_against_python_integers():
    """The int64 reference itself, against the definition in Python integers on a ragged rank-3 case with a cap."""
    rng = np.random.default_rng(5)
    x, y, zs = rng.integers(-3, 4, size=(3, 4, 2)), rng.integers(-3, 4, size=(2, 3, 4)), (4, 5, 4)
    want = np.zeros(zs, dtype=object)
    for i in np.ndindex(x.shape):
        for j in np.ndindex(y.shape):
            k = tuple(a + b for a, b in zip(i, j))
            if all(c < z for c, z in zip(k, zs)):
                want[k] += int(x[i]) * int(y[j])
    assert np.array_equal(int_conv(x, y, zs), want.astype(np.int64))
    assert np.array_equal(int_conv(y, x, zs), want.astype(np.int64))


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_magnitude_bounds_and_crossover_on_the_oracle(name, OTP):
    """The generator's bookkeeping against the actual trees, on the oracle alone: at every node of every seeded tree the
    coefficients are integers with max |coeff| <= B < 2^53 (so the tree is exact in any summation order), the leaf-level
    products equal the plain int64 convolution, and the trees do reach the kernels under test: 62 of the 64 seeded trees
    (16 classes x 4 seeds; TREES_WITH_TILED per class) contain at least one product that the automatic dispatch sends to the
    tiled kernel (_exact_int.product_path, the dispatcher's arithmetic on the stored shapes) — the issue's 90 % is 58."""
    hit = 0
    for gen, root in _trees(name, [OTP], check_nodes=True):
        assert root.B < LIMIT
        _check_leaf_products(gen, 0)
        hit += any(path == "tiled" for path, _ in gen.products)
    assert hit >= 1
    assert hit >= TREES_WITH_TILED[name], (name, hit)


# trees (of SEEDS = 4 per class) that contain a product at or above the crossover, counted by the test above
TREES_WITH_TILED = {name: SEEDS - (name in ("rank3_inner8", "rank4")) for name in CLASSES}  # 62 of 64


def test_nine_trees_in_ten_cross_the_crossover():
    assert sum(TREES_WITH_TILED.values()) >= 0.9 * SEEDS * len(CLASSES)


@contextlib.contextmanager
def _options(opts):
    import genfer_amd

    L = genfer_amd.lib()
    try:
        for k, (v, _) in opts.items():
            assert L.gft_set_option(k, float(v)) == 0
        yield
    finally:
        for k, (_, restore) in opts.items():
            assert L.gft_set_option(k, float(restore)) == 0


def _run_class(name, OTP, GTP, tier, extra_options=None):
    import genfer_amd

    cls = CLASSES[name]
    opts = dict(cls.get("options", {}))
    opts.update(extra_options or {})
    with _options(opts):
        before = genfer_amd.op_stats()
        for gen, root in _trees(name, [OTP, GTP]):
            o, g = root.h
            assert o.coeffs_shape() == g.coeffs_shape() and o.degrees_p1() == g.degrees_p1(), (o.coeffs_shape(), g.coeffs_shape(), o.degrees_p1(), g.degrees_p1())
            a, b = np.asarray(o.array()), np.asarray(g.array())
            assert not np.isnan(b).any(), "NaN in an exact integer tree"
            assert np.array_equal(a, b), (name, np.argwhere(a != b)[:4], a[a != b][:4], b[a != b][:4])
            _check_leaf_products(gen, 1)
        after = genfer_amd.op_stats()
    delta = {k: after[k] - before[k] for k in ("tiled", "tiled_peeled", "shallow_products", "staged", "per_output", "launches")}
    print(name, tier, delta)
    if tier == "device":  # the host tier asserts only the values
        assert delta["tiled"] >= 1, delta
        for counter in cls.get("expect", ()):
            assert delta[counter] >= 1, (counter, delta)
    return delta


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["device", "host"], indirect=True)
@pytest.mark.parametrize("name", sorted(CLASSES))
def test_exact_integer_trees(name, tier, OTP, GTP):
    """Every shape class: SEEDS trees of depth <= 3 through the handle API in auto mode equal the oracle value for value,
    their leaf-level products equal the int64 convolution, and (device tier) op_stats shows that the class's kernel ran:
    `tiled` rises in every class, `tiled_peeled` in the peel class, `shallow_products` where a compact operand makes a
    product shallow."""
    _run_class(name, OTP, GTP, tier)


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["device", "host"], indirect=True)
@pytest.mark.parametrize("defer", [1, 0], ids=["deferred", "launched"])
def test_exact_integer_trees_deferred_and_launched(defer, tier, OTP, GTP):
    """One class with the deferred launch graph on and off (elementwise results as chain stages / one launch each)."""
    _run_class("rank3_inner28", OTP, GTP, tier, {b"defer": (defer, 1)})


@pytest.mark.gpu
def test_exact_products_of_products_read_in_place(OTP, GTP):
    """Operands that are themselves results of products sit in library buffers (64 bytes of slack) with rows of whole
    8-coefficient chunks: the tiled kernel reads them in place — one tiled product, at most the main kernel and its
    reduce launched, no packing launch — and the integer result is exact."""
    import genfer_amd

    rng = np.random.default_rng(77)
    deg = CLASSES["rank3_in_place"]["deg"]
    leaves = [rng.integers(-3, 4, size=s).astype(np.float64) for s in [(12, 11, 16), (12, 11, 17)] * 2]
    assert np.prod([np.abs(a).sum() for a in leaves]) < LIMIT
    o = [OTP.new(a, deg) for a in leaves]
    g = [GTP.new(a, deg) for a in leaves]
    po, qo, pg, qg = o[0] * o[1], o[2] * o[3], g[0] * g[1], g[2] * g[3]
    assert tuple(pg.coeffs_shape()) == tuple(deg) == tuple(qg.coeffs_shape())
    (pg * qg).array()  # extract_linear verdicts are memoised on the operands' buffers now
    before = genfer_amd.op_stats()
    got = pg * qg
    after = genfer_amd.op_stats()
    assert after["tiled"] - before["tiled"] == 1
    assert after["launches"] - before["launches"] <= 2, "in-place operands: the main kernel and the reduce, nothing else"
    want = np.asarray((po * qo).array())
    assert np.array_equal(want, np.asarray(got.array()))
    # ... and against the int64 convolution end to end
    p = int_conv(leaves[0], leaves[1], tuple(deg))
    q = int_conv(leaves[2], leaves[3], tuple(deg))
    assert np.array_equal(int_conv(p, q, tuple(deg)).astype(np.float64), np.asarray(got.array()))
