"""Fixed programs over interval handles, one family per rule of the zero-pattern proofs.

Every case is a straight-line program written once against the class `bind()` produces, so the same function runs on the CPU
oracle (tests/test_support_cases_cpu.py: the true zero pattern of every probed step is the one stated here) and on the GPU
(tests/test_support_claims_gpu.py: the library's claim for every probed step holds for the oracle's data of that step).

A case calls `R.probe(name, handle, want)` right after the step that produced `handle`; `want` is the boolean array of the
coefficients that are exactly [0,0], worked out here with numpy slicing from the planted pattern of the inputs — never from
either backend.  `R.keep(name, value)` records a host-visible answer (extract_linear, constant_term, is_zero)."""
import numpy as np

from conftest import splitmix64_uniform

ZERO, NZ, STRADDLE, INF = (0.0, 0.0), (0.5, 0.75), (-0.5, 0.25), (1.0, float("inf"))
SCALARS = {"zero": ZERO, "nz": NZ, "straddle": STRADDLE, "inf": INF}
R9 = (4, 1, 1, 1, 1, 1, 1, 1, 16)  # rank 9 with unit axes: axis index 8 is beyond what a claim can speak about

CASES = []


class Case:
    def __init__(self, family, fn, options, proofs, boundary):
        self.family, self.fn, self.name = family, fn, fn.__name__
        self.options = options      # option settings the GPU test runs the case under, besides the defaults
        self.proofs = proofs        # also run with nz_proofs = 0 and compare bit for bit
        self.boundary = boundary    # ((probe, predicate), ..): probes whose TRUE zero pattern sits on the rule's edge, checked on the oracle


def case(family, options=(), proofs=True, boundary=()):
    def reg(fn):
        CASES.append(Case(family, fn, tuple(options), proofs, tuple(boundary)))
        return fn
    return reg


def families():
    out = []
    for c in CASES:
        if c.family not in out:
            out.append(c.family)
    return out


class Run:
    """One execution of a case on one backend.  `claim`: reads the library's claim of a handle (GPU runs), else None."""

    def __init__(self, T, claim=None):
        self.T, self.claim = T, claim
        self.probes, self.kept, self.held = [], [], []

    def probe(self, name, h, want):
        self.probes.append({"name": name, "h": h, "want": np.asarray(want, dtype=bool),
                            "claim": self.claim(h) if self.claim else None})
        return h

    def keep(self, name, value):
        self.kept.append((name, value))

    def hold(self, name, h):
        """a handle whose value is compared at the end, without a stated zero pattern"""
        self.held.append((name, h))

    def finish(self):
        """Consumers: every probed tensor that is not tiny goes through a proven subst_var along its longest axis and through
        extract_linear(), then everything is read back: {name: (degrees_p1, array)} and the kept answers."""
        T = self.T
        cons = []
        for p in list(self.probes):
            h = p["h"]
            shape = h.coeffs_shape()
            if int(np.prod(shape)) < 64:
                continue
            v = int(np.argmax(shape))
            r = h.subst_var(v, proven_subst(T, v, h.degrees_p1()))
            self.keep(p["name"] + ".extract_linear", h.extract_linear())
            self.keep(p["name"] + ".subst.extract_linear", r.extract_linear())
            cons.append((p["name"] + ".subst", r))
            p["claim_after"] = self.claim(h) if self.claim else None
        out = {}
        for name, h in [(p["name"], p["h"]) for p in self.probes] + cons + self.held:
            assert name not in out, name
            out[name] = (h.degrees_p1(), np.asarray(h.array()))
        return out, list(self.kept)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def planes(shape, seed, zero=None):
    """lo in [0.05, 0.95), hi = lo + 1/8, exact zeros where `zero` (a boolean array) says."""
    u = splitmix64_uniform(seed, int(np.prod(shape))).reshape(shape)
    lo = 0.05 + 0.9 * u
    hi = lo + 0.125
    if zero is not None:
        lo[zero], hi[zero] = 0.0, 0.0
    return np.stack([lo, hi])


def none(shape):
    return np.zeros(shape, dtype=bool)


def every(shape):
    return np.ones(shape, dtype=bool)


def slabs(shape, z):
    """k_u < z[u] for some u"""
    m = np.zeros(shape, dtype=bool)
    idx = np.indices(shape)
    for u, n in z.items():
        m |= idx[u] < n
    return m


def outside(shape, lo, hi):
    idx = np.indices(shape)
    inside = np.ones(shape, dtype=bool)
    for u in range(len(shape)):
        inside &= (idx[u] >= lo[u]) & (idx[u] < hi[u])
    return ~inside


def prod_mask(za, zb, shape):
    """a * b: interval products do not cancel, so coefficient k is [0,0] iff no pair of non-zero coefficients meets there"""
    nz = np.zeros(shape, dtype=bool)
    for i in np.argwhere(~za):
        for j in np.argwhere(~zb):
            k = i + j
            if np.all(k < shape):
                nz[tuple(k)] = True
    return ~nz


def mk(T, shape, seed, zero=None, deg=None):
    return T.new(planes(shape, seed, zero), list(deg or shape))


def proven_subst(T, v, deg, c=(0.25, 0.25), m=(0.5, 0.5)):
    """c * m + m * x_v as a 2-element substitution whose constant term is a non-zero finite interval: the Horner loop on an
    interval tensor is then PROVEN, which is what makes the library ask for a tensor's zero pattern."""
    return T.var_with_degrees_p1(v, c, list(deg)) * T.from_scalar(m)


def measure(T, p, v):
    """A proven subst_var on p along v: the library measures p's zero pattern (p of >= 64 coefficients) on the way."""
    return p.subst_var(v, proven_subst(T, v, p.degrees_p1()))


def measured(T, R, name, shape, seed, zero=None, v=0, deg=None):
    z = none(shape) if zero is None else zero
    p = mk(T, shape, seed, zero, deg)
    measure(T, p, v)
    R.probe(name, p, z)
    return p, z


def zeros_measured(T, R, name, shape, v=0):
    return measured(T, R, name, shape, 0, every(shape), v)


def slabbed(T, R, name, shape, seed, axis, z):
    """A tensor whose exact zeros are the leading z slabs of `axis`, built the way programs build it: multiply by the variable
    (a front pad) and add an all-zero tensor, z times.  Returns (handle, mask)."""
    cur, _ = measured(T, R, name + ".z0", shape, seed, v=1 - axis if len(shape) == 2 else (axis + 1) % len(shape))
    zt, _ = zeros_measured(T, R, name + ".zeros", shape)
    for k in range(1, z + 1):
        cur = cur.mul_var(NZ, axis, list(shape), list(shape)) + zt
        R.probe(f"{name}.z{k}", cur, slabs(shape, {axis: k}))
    return cur, slabs(shape, {axis: z})


def scaled(R, name, T, h, Z, cls, how):
    """One elementwise stage with a scalar of class `cls`; returns (handle, true mask)."""
    s = SCALARS[cls]
    r = {"mul": lambda: h * T.from_scalar(s), "lmul": lambda: T.from_scalar(s) * h, "div": lambda: h / T.from_scalar(s)}[how]()
    if how == "div":
        # x / [0,0] is NaN for x = [0,0] and unbounded otherwise; [0,0] / s is [0,0] for every other s (iv:199-234)
        want = none(Z.shape) if cls == "zero" else Z
    else:
        # [0,0] * s is [0,0] for finite s only (iv:164-190): with an infinite bound it is NaN
        # (Mul returns the 1-element zero polynomial for a zero factor, mt:1014-1020)
        want = every(r.coeffs_shape()) if cls == "zero" else (none(Z.shape) if cls == "inf" else Z)
    R.probe(name, r, want)
    return r, want


# ---- measurement [nz_query] ---------------------------------------------------------------------------------------------------
@case("measurement")
def measure_no_zero(T, R):
    p = mk(T, (6, 12), 11)
    R.probe("p.unasked", p, none((6, 12)))
    r = measure(T, p, 1)
    R.probe("p", p, none((6, 12)))
    R.probe("r", r, none(r.coeffs_shape()))


@case("measurement", boundary=(("r1", lambda m: not m.any()),))
def measure_slab0_of_one_axis(T, R):
    z = slabs((6, 12), {1: 1})
    p = mk(T, (6, 12), 12, z)
    r = measure(T, p, 0)                       # the slab lies across the substituted axis: it stays
    R.probe("p", p, z)
    R.probe("r", r, slabs(r.coeffs_shape(), {1: 1}))
    r1 = measure(T, p, 1)                      # the slab is the constant coefficient of the substituted axis: it fills up
    R.probe("r1", r1, none(r1.coeffs_shape()))


@case("measurement", boundary=(("r", lambda m: m[0].all() and m[:, :, 0].all() and not m[1:, :, 1:].any()),))
def measure_slab0_of_two_axes(T, R):
    z = slabs((4, 5, 6), {0: 1, 2: 1})
    p = mk(T, (4, 5, 6), 13, z)
    r = measure(T, p, 1)
    R.probe("p", p, z)
    R.probe("r", r, slabs(r.coeffs_shape(), {0: 1, 2: 1}))


@case("measurement", boundary=(("p", lambda m: m[0].all() and m[1:].sum() == 1),))
def measure_slab0_plus_a_stray_zero(T, R):
    z = slabs((6, 12), {0: 1})
    z[3, 5] = True                             # not a slab pattern: must not become "exactly the leading slabs"
    p = mk(T, (6, 12), 14, z)
    measure(T, p, 1)
    R.probe("p", p, z)
    q = p.coefficients_of_term(0, 3)
    R.probe("q", q, z[3:4])


@case("measurement", boundary=(("p", lambda m: m[0].sum() == 11 and not m[1:].any()),))
def measure_denormal_bound_is_not_a_zero(T, R):
    a = planes((6, 12), 15, slabs((6, 12), {0: 1}))
    a[1, 0, 3] = 5e-324                        # [0, 5e-324] inside the zero slab
    z = slabs((6, 12), {0: 1})
    z[0, 3] = False
    b = planes((6, 12), 16)
    b[0, 2, 2], b[1, 2, 2] = 0.0, 5e-324       # ... and alone in a tensor without zeros
    p2 = T.new(b, [6, 12])
    measure(T, p2, 1)
    R.probe("p2", p2, none((6, 12)))
    p = T.new(a, [6, 12])
    measure(T, p, 1)
    R.probe("p", p, z)


@case("measurement", boundary=(("p", lambda m: m.all()),))
def measure_all_zero(T, R):
    p, z = zeros_measured(T, R, "p", (6, 12))
    R.probe("neg", -p, z)
    R.probe("box", p.coefficients_of_term(0, 2), z[2:3])


@case("measurement")
def measure_pending_chain_asks_its_base(T, R):
    z = slabs((6, 12), {1: 1})
    p = mk(T, (6, 12), 17, z)
    q = p * T.from_scalar(NZ)                  # a deferred stage: the handle is not asked, its base tensor is
    r = measure(T, q, 0)
    R.probe("p", p, z)
    R.probe("q", q, z)
    R.probe("r", r, slabs(r.coeffs_shape(), {1: 1}))


@case("measurement")
def measure_rank9(T, R):
    p = mk(T, R9, 18)
    measure(T, p, 8)
    R.probe("p", p, none(R9))
    z = slabs(R9, {8: 1})
    q = mk(T, R9, 19, z)
    measure(T, q, 0)
    R.probe("q", q, z)                          # zeros on an axis no claim can name


# ---- observe_chain [gft_ops_observe.inc, Support of a chain's result] --------------------------------------------------------------
def _observe(T, R, tag, a, Z, v, x, n):
    shape = a.coeffs_shape()
    d = max(shape)
    r = a.observe_chain(v, x, [NZ] * n, d)
    zs = Z
    for _ in range(n):  # derivative: slabs of axis v move down by one; (x + eps_v) *: stay (x not zero) or move up by one (x zero)
        zd = np.delete(zs, 0, axis=v)
        pad = np.ones_like(np.take(zd, [0], axis=v))
        up = np.concatenate([pad, zd], axis=v)              # D[k - 1], zero for k = 0
        here = np.concatenate([zd, pad], axis=v)            # D[k], zero past the end
        zs = up if x == ZERO else (up & here)
    lead = tuple(slice(0, s) for s in r.coeffs_shape())
    R.probe(tag, r, zs[lead])
    return r


def _observe_family(zv):
    def run(T, R):
        shape = (6, 12)
        if zv == 0:
            a, Z = measured(T, R, "a", shape, 21, v=0)
        elif zv == 1:
            a, Z = measured(T, R, "a", shape, 22, slabs(shape, {1: 1}), v=0)
        else:
            a, Z = slabbed(T, R, "a", shape, 23, 1, 2)
        for xn, x in (("x0", ZERO), ("xnz", NZ)):
            for n in (1, 3):
                _observe(T, R, f"obs.{xn}.n{n}", a, Z, 1, x, n)
        # x with an infinite bound: out[0] = x * D[0], and x * [0,0] is NaN — where the derivative still has a zero slab (two
        # slabs in the input) the result holds NaN there, not [0,0]
        r = a.observe_chain(1, INF, [NZ], 12)
        R.probe("obs.xinf.n1", r, none(r.coeffs_shape()))
    run.__name__ = f"observe_input_slabs_{zv}"
    return run


for _zv in (0, 1, 2):
    case("observe_chain", options=({"lazy_observe": 0},), boundary=((("obs.x0.n1", lambda m: m[:, :2].all() and not m[:, 2:].any()),) if _zv == 2 else ()))(_observe_family(_zv))


@case("observe_chain", options=({"lazy_observe": 0},), boundary=(("r", lambda m: m.all() and m.shape == (32, 1)), ("b.x0.n2", lambda m: m[:, 0].all() and not m[:, 1:].any())))
def observe_slabs_swallow_the_box(T, R):
    a, Z = measured(T, R, "a", (32, 2), 24, v=0, deg=[32, 2])
    r = a.observe_chain(1, ZERO, [NZ], 32)     # D * eps_1 cut back to one coefficient along axis 1: nothing but zeros
    R.probe("r", r, every(r.coeffs_shape()))
    b, Zb = measured(T, R, "b", (22, 3), 25, v=0, deg=[22, 3])
    _observe(T, R, "b.x0.n1", b, Zb, 1, ZERO, 1)
    _observe(T, R, "b.x0.n2", b, Zb, 1, ZERO, 2)


@case("observe_chain", options=({"lazy_observe": 0},))
def observe_axis_beyond_the_claim(T, R):
    a, Z = measured(T, R, "a", R9, 26, v=0)
    _observe(T, R, "x0", a, Z, 8, ZERO, 1)
    _observe(T, R, "xnz", a, Z, 8, NZ, 1)
    _observe(T, R, "axis0.x0", a, Z, 0, ZERO, 1)


# ---- sub-boxes and elementwise stages [gather's rule; support_of_poly's pend branch] -----------------------------------------------
def _boxes(T, R, tag, p, Z, ax):
    """Every one-slab box of p along ax, the leading boxes, derivative and shift_down; stages on a box past the origin."""
    n = p.coeffs_shape()[ax]
    out = []
    for k in range(min(n, 5)):
        c = p.coefficients_of_term(ax, k)
        zc = np.take(Z, [k], axis=ax)
        R.probe(f"{tag}.term{k}", c, zc)
        out.append((c, zc))
    t = p.taylor_polynomial_terms(ax, [1, 3])
    zt = np.take(Z, range(4), axis=ax).copy()
    sl = [slice(None)] * Z.ndim
    for k in (0, 2):
        sl[ax] = k
        zt[tuple(sl)] = True
    R.probe(f"{tag}.terms13", t, zt)
    for d in (1, 2, 4):
        lead = tuple(slice(0, min(d, s)) for s in Z.shape)
        R.probe(f"{tag}.trunc{d}", p.truncate_to_degree_p1(d), Z[lead])
    for k in (1, 2):
        R.probe(f"{tag}.deriv{k}", p.derivative(ax, k), np.delete(Z, range(k), axis=ax))
    zs = np.delete(Z, 0, axis=ax)
    sl[ax] = 0
    zs[tuple(sl)] &= np.take(Z, 0, axis=ax)    # slab 0 of the result is c[0] + c[1]: zero only where both are
    R.probe(f"{tag}.shift1", p.shift_down(ax, 1), zs)
    return out


def _stages(T, R, tag, h, Z):
    for how in ("mul", "lmul", "div"):
        for cls in SCALARS:
            r, zr = scaled(R, f"{tag}.{how}.{cls}", T, h, Z, cls, how)
            if cls == "nz":
                R.probe(f"{tag}.{how}.{cls}.neg", -r, zr)
    R.probe(f"{tag}.neg", -h, Z)


def _subbox_program(zv, ax):
    def run(T, R):
        shape = (6, 12)
        if zv < 2:
            p, Z = measured(T, R, "p", shape, 31 + zv, slabs(shape, {ax: 1}) if zv else None, v=1 - ax)
        else:
            p, Z = slabbed(T, R, "p", shape, 33, ax, 2)
        bx = _boxes(T, R, "p", p, Z, ax)
        _stages(T, R, "whole", p, Z)
        for k in (zv - 1, zv, zv + 1):          # the box lies in the last zero slab, starts right behind it, one further
            if 0 <= k < len(bx):
                _stages(T, R, f"term{k}", bx[k][0], bx[k][1])
        other = p.coefficients_of_term(1 - ax, 2)   # a box across the slabs, off the origin on the other axis
        zo = np.take(Z, [2], axis=1 - ax)
        R.probe("across", other, zo)
        _stages(T, R, "across", other, zo)
    run.__name__ = f"boxes_and_stages_slabs{zv}_axis{ax}"
    return run


for _zv, _ax in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1)):
    # "defer" off: every box and stage is a gather into a fresh tensor (the gather's rule); on: a view with stages (the chain rule)
    case("boxes_and_stages", options=({"defer": 0},), boundary=(((f"p.term{_zv - 1}", lambda m: m.all()), (f"p.term{_zv}", lambda m: not m.any())) if _zv > 0 else ()))(_subbox_program(_zv, _ax))


@case("boxes_and_stages", options=({"defer": 0},))
def boxes_rank4_and_rank9(T, R):
    sh = (3, 4, 3, 4)
    p, Z = measured(T, R, "p4", sh, 36, slabs(sh, {1: 1, 3: 1}), v=0)
    c = p.coefficients_of_term(1, 1)
    R.probe("p4.term1", c, Z[:, 1:2])
    _stages(T, R, "p4.term1", c, Z[:, 1:2])
    c0 = p.coefficients_of_term(3, 0)
    R.probe("p4.swallowed", c0, Z[..., 0:1])
    q, Zq = measured(T, R, "p9", R9, 37, v=0)
    c9 = q.coefficients_of_term(8, 3)
    R.probe("p9.term3", c9, np.take(Zq, [3], axis=8))
    R.probe("p9.trunc2", q.truncate_to_degree_p1(2), Zq[:2, ..., :2])


@case("chains", boundary=(("p1.scale.zero", lambda m: m.all()),))
def chain_scaling_tables(T, R):
    """MUL_TAB: the scaling substitution x_v -> m * x_v multiplies slab k by m^k."""
    shape = (6, 12)
    for zv, seed in ((0, 41), (1, 42)):
        p, Z = measured(T, R, f"p{zv}", shape, seed, slabs(shape, {1: 1}) if zv else None, v=0)
        for cls in ("nz", "straddle", "zero"):
            m = SCALARS[cls]
            sub = T.new(np.array([[0.0, m[0]], [0.0, m[1]]]).reshape(2, 1, 2), [6, 12])  # 0 + m * x_1
            r = p.subst_var(1, sub)
            zr = Z.copy()
            if cls == "zero":
                zr[:, 1:] = True               # m^0 = 1 keeps slab 0, every higher power of [0,0] is [0,0]
            lead = tuple(slice(0, s) for s in r.coeffs_shape())
            R.probe(f"p{zv}.scale.{cls}", r, zr[lead])
            if cls != "zero":
                c = r.coefficients_of_term(1, 1)
                R.probe(f"p{zv}.scale.{cls}.term1", c, zr[:, 1:2])


@case("chains", boundary=(("k3.plus_nz", lambda m: not m[0, 0] and m[1:, 0].all() and not m[:, 1:].any()),))
def chain_first_element_stages(T, R):
    """FIRST_ADD / FIRST_SUB: `p - constant_term(p)` (the interpreter's idiom) and `p + s`, on tensors without zeros, with
    leading slabs (element 0 lies in one) and all zero."""
    shape = (6, 12)
    p2, Z2 = measured(T, R, "k2", shape, 43, v=0)
    p3, Z3 = measured(T, R, "k3", shape, 44, slabs(shape, {1: 1}), v=0)
    p5, Z5 = zeros_measured(T, R, "k5", shape)
    for tag, p, Z in (("k2", p2, Z2), ("k3", p3, Z3), ("k5", p5, Z5)):
        c = p.constant_term()
        R.keep(f"{tag}.c0", c)
        r = p - T.from_scalar(c)
        zr = Z.copy()                           # x - x is widened (not zero) unless x is [0,0], and then [0,0] - [0,0] is [0,0]
        R.probe(f"{tag}.minus_c0", r, zr)
        R.keep(f"{tag}.minus_c0.c0", r.constant_term())
        for name, s, f in (("plus_nz", NZ, lambda a, b: a + b), ("minus_nz", NZ, lambda a, b: a - b), ("rsub_nz", NZ, lambda a, b: b - a),
                           ("plus_zero", ZERO, lambda a, b: a + b), ("rsub_zero", ZERO, lambda a, b: b - a)):
            r = f(p, T.from_scalar(s))
            zr = Z.copy()
            if s != ZERO:
                zr[0, 0] = False               # [0,0] + s is s; a non-zero element plus s is widened
            R.probe(f"{tag}.{name}", r, zr)
            R.probe(f"{tag}.{name}.scaled", r * T.from_scalar(NZ), zr)
            if tag == "k3":
                R.probe(f"{tag}.{name}.row0", r.coefficients_of_term(0, 0), zr[0:1])


# ---- front padding [mul_var: kind 4] ---------------------------------------------------------------------------------------------
def _mul_var_mask(Z, v, shape):
    """mt:589-608: the operand's leading slabs of axis v, moved up by one inside the result's box; zero elsewhere"""
    out = np.ones(shape, dtype=bool)
    upper = min(shape[v] - 1, Z.shape[v])
    lens = [min(a, b) for a, b in zip(Z.shape, shape)]
    lens[v] = upper
    src = Z[tuple(slice(0, n) for n in lens)]
    dst = [slice(0, n) for n in lens]
    dst[v] = slice(1, 1 + upper)
    out[tuple(dst)] = src
    return out


@case("padding", boundary=(("k3.same", lambda m: m[:, :2].all() and not m[:, 2:].any()), ("k3.two", lambda m: m.all())))
def pads_on_plain_and_slabbed_tensors(T, R):
    shape = (6, 12)
    p2, Z2 = measured(T, R, "k2", shape, 51, v=0)
    p3, Z3 = measured(T, R, "k3", shape, 52, slabs(shape, {1: 1}), v=0)
    for tag, p, Z in (("k2", p2, Z2), ("k3", p3, Z3)):
        for name, v, sh in (("same", 1, (6, 12)), ("longer", 1, (6, 13)), ("narrower", 1, (4, 12)), ("behind", 1, (8, 13)),
                            ("axis0", 0, (6, 12)), ("two", 1, (6, 2)), ("three", 1, (6, 3))):
            q = p.mul_var(NZ, v, list(sh), list(sh))
            zq = _mul_var_mask(Z, v, sh)
            R.probe(f"{tag}.{name}", q, zq)
            if name in ("same", "behind"):
                q2 = q.mul_var(NZ, v, list(sh), list(sh))   # a pad on a pad
                R.probe(f"{tag}.{name}.twice", q2, _mul_var_mask(zq, v, sh))
                s = q * T.from_scalar(NZ)                      # a stage attempted after a pad
                R.probe(f"{tag}.{name}.scaled", s, zq)
                s0 = q * T.from_scalar(ZERO)                   # (Mul's zero shortcut: the 1-element zero polynomial)
                R.probe(f"{tag}.{name}.scaled0", s0, every(s0.coeffs_shape()))
                R.probe(f"{tag}.{name}.term1", q.coefficients_of_term(v, 1), np.take(zq, [1], axis=v))
        view = p.coefficients_of_term(0, 2) * T.from_scalar(NZ)  # a view off the origin with a stage, then the pad
        zv = Z[2:3]
        R.probe(f"{tag}.view.pad", view.mul_var(NZ, 1, [1, 12], [6, 12]), _mul_var_mask(zv, 1, (1, 12)))


@case("padding")
def pad_on_an_axis_beyond_the_claim(T, R):
    p, Z = measured(T, R, "p", R9, 53, v=0)
    R.probe("pad8", p.mul_var(NZ, 8, list(R9), list(R9)), _mul_var_mask(Z, 8, R9))
    R.probe("pad0", p.mul_var(NZ, 0, list(R9), list(R9)), _mul_var_mask(Z, 0, R9))


# ---- materialisation [settle, recorded_settle] ------------------------------------------------------------------------------------
@case("materialisation", boundary=(("swallowed.settled", lambda m: m.all()), ("off.settled", lambda m: not m.any())))
def chains_keep_their_claim_when_materialised(T, R):
    shape = (6, 12)
    p, Z = measured(T, R, "p", shape, 61, slabs(shape, {1: 1}), v=0)
    for tag, q, zq in (("lead", p.truncate_to_degree_p1(5) * T.from_scalar(NZ), Z[:5, :5]),
                       ("off", -p.coefficients_of_term(1, 1), Z[:, 1:2]),
                       ("swallowed", p.coefficients_of_term(1, 0) * T.from_scalar(NZ), Z[:, 0:1]),
                       ("whole", T.from_scalar(NZ) * p, Z),
                       ("pad", p.mul_var(NZ, 1, [6, 12], [6, 12]), _mul_var_mask(Z, 1, shape))):
        twin = q.clone()
        R.probe(f"{tag}.chain", q, zq)
        prod = q * q                           # a product reads its operands from memory: the chain is materialised
        R.probe(f"{tag}.settled", q, zq)
        R.probe(f"{tag}.twin", twin, zq)
        R.probe(f"{tag}.again", twin * T.from_scalar(NZ), zq)
        R.probe(f"{tag}.prod", prod, prod_mask(zq, zq, prod.coeffs_shape()))


@case("materialisation", options=({"batch_dag": 0}, {"lazy_observe": 0}))
def chain_as_the_input_of_an_observation(T, R):
    shape = (6, 12)
    p, Z = measured(T, R, "p", shape, 62, v=0)
    q = p * T.from_scalar(NZ)
    _observe(T, R, "obs.x0", q, Z, 1, ZERO, 1)
    _observe(T, R, "obs.xnz", q, Z, 1, NZ, 2)
    R.probe("q", q, Z)


# ---- sums [sum_support] ---------------------------------------------------------------------------------------------------------------
def _sum(R, name, a, za, b, zb, sub=False):
    """a (+|-) b: [0,0] exactly where both are (a smaller operand counts as zero outside its own shape)"""
    r = (a - b) if sub else (a + b)
    sh = r.coeffs_shape()

    def ext(z):
        z = z.reshape(z.shape + (1,) * (len(sh) - z.ndim))
        out = np.ones(sh, dtype=bool)
        out[tuple(slice(0, n) for n in z.shape)] = z
        return out
    R.probe(name, r, ext(za) & ext(zb))
    return r, ext(za) & ext(zb)


def _sums(sub):
    def run(T, R):
        shape = (6, 12)
        full, zf = measured(T, R, "full", shape, 71, v=0)
        zeros, zz = zeros_measured(T, R, "zeros", shape)
        z1, m1 = measured(T, R, "z1", shape, 72, slabs(shape, {0: 1}), v=1)
        rows = {}
        for k in (2, 3, 4):
            rows[k] = slabbed(T, R, f"rows{k}", shape, 73 + k, 0, k)
        top, zt = measured(T, R, "top", (3, 12), 78, v=1, deg=shape)     # non-zero on rows [0, 3)
        left, zl = measured(T, R, "left", (6, 5), 79, v=0, deg=shape)    # non-zero on columns [0, 5)
        padded = full.mul_var(NZ, 1, list(shape), list(shape))           # columns [1, 12)
        zp = _mul_var_mask(zf, 1, shape)
        cols2, mc2 = slabbed(T, R, "cols2", shape, 80, 1, 2)
        s = T.from_scalar(NZ)
        _sum(R, "full+slabs", full * s, zf, z1 * s, m1, sub)                      # one operand full: no zero
        _sum(R, "slabs+full", z1 * s, m1, full * s, zf, sub)
        _sum(R, "contains", z1 * s, m1, rows[2][0] * s, rows[2][1], sub)          # one contains the other: the larger box
        _sum(R, "contained", rows[3][0] * s, rows[3][1], z1 * s, m1, sub)
        _sum(R, "overlap", top * s, zt, rows[2][0] * s, rows[2][1], sub)          # rows [0,3) and [2,6)
        _sum(R, "touch", top * s, zt, rows[3][0] * s, rows[3][1], sub)            # rows [0,3) and [3,6): just touching
        _sum(R, "gap", top * s, zt, rows[4][0] * s, rows[4][1], sub)              # rows [0,3) and [4,6): row 3 stays zero
        _sum(R, "L", top * s, zt, left * s, zl, sub)                              # boxes differing on two axes
        _sum(R, "L2", z1 * s, m1, cols2 * s, mc2, sub)
        _sum(R, "empty", zeros * s, zz, -zeros, zz, sub)                          # both empty: all zero
        _sum(R, "empty+slabs", zeros * s, zz, z1 * s, m1, sub)
        _sum(R, "pad.contained", padded, zp, full * s, zf, sub)                   # a padded operand inside the other
        _sum(R, "pad.containing", padded, zp, cols2 * s, mc2, sub)               # ... and around it
        _sum(R, "pad.meets", padded, zp, zeros * s, zz, sub)
        _sum(R, "pad.L", padded, zp, z1 * s, m1, sub)
        _sum(R, "broadcast", (full * s).extend_to_dim(3, 4), zf, z1 * s, m1, sub)  # operands of different rank
        _sum(R, "plain", full, zf, z1, m1, sub)                                   # no chain on either side
    run.__name__ = "sums_of_boxes_" + ("sub" if sub else "add")
    return run


for _sub in (False, True):
    case("sums", options=({"lazy_sum": 0}, {"batch_dag": 0}), boundary=(("touch", lambda m: not m.any()), ("gap", lambda m: m[3].all() and m.sum() == 12)))(_sums(_sub))


@case("sums", options=({"lazy_sum": 0}, {"batch_dag": 0}))
def sums_recorded_and_nested(T, R):
    """mul_linear's Add (c * t + m * shift(t)) is a recorded two-chain sum; the merge of two of them is the nested Add."""
    shape = (2, 8, 8)
    ta, za = measured(T, R, "ta", shape, 81, v=1)
    tb, zb = measured(T, R, "tb", shape, 82, slabs(shape, {2: 1}), v=1)
    s1 = ta.mul_linear((0.8, 0.8), (0.2, 0.2), 0, list(shape), list(shape))
    s2 = tb.mul_linear((0.3, 0.3), (0.7, 0.7), 0, list(shape), list(shape))
    R.probe("s1", s1, za)
    R.probe("s2", s2, zb)
    R.probe("merged", s1 + s2, za & zb)
    R.probe("again", s1 - tb, za & zb)
    s3 = tb.mul_linear(ZERO, (0.7, 0.7), 0, list(shape), list(shape))          # c = 0: the pad alone
    R.probe("s3", s3, _mul_var_mask(zb, 0, shape))
    R.probe("s3+s2", s3 + s2, _mul_var_mask(zb, 0, shape) & zb)


# ---- Horner results [horner_linear_rest] --------------------------------------------------------------------------------------------
@case("horner", options=({"lazy_horner": 0}, {"batch_dag": 0}), boundary=(("on_axis.r", lambda m: not m.any()), ("on_axis.cross_c0", lambda m: m[0].all() and not m[1:].any()), ("other_axis.cross_c0", lambda m: m[0].all() and not m[1:].any())))
def proven_loops(T, R):
    shape = (6, 12)
    for tag, zero in (("k2", None), ("on_axis", {1: 1}), ("other_axis", {0: 1})):
        Z = slabs(shape, zero) if zero else none(shape)
        p, _ = measured(T, R, tag, shape, 91 + len(tag), Z if zero else None, v=0 if tag != "other_axis" else 1)
        r = measure(T, p, 1)                  # x_1 -> c + m x_1: along x_1 the top coefficient reaches every position
        R.probe(f"{tag}.r", r, slabs(r.coeffs_shape(), {0: 1}) if tag == "other_axis" else none(r.coeffs_shape()))
        r2 = measure(T, r, 0)                 # a loop on a loop's result
        R.probe(f"{tag}.r2", r2, none(r2.coeffs_shape()))
        w = p.subst_var(1, proven_subst(T, 0, [6, 12]))     # x_1 -> c + m x_0: another variable
        zw = slabs(w.coeffs_shape(), {0: 1}) if tag == "other_axis" else none(w.coeffs_shape())  # x_0^0 collects row 0 alone
        R.probe(f"{tag}.cross", w, zw)
        # x_1 -> [0,0] + m x_0 (c zero, another variable: a Horner loop, not the scaling table): x_0^0 receives a[0,0] alone,
        # which is [0,0] as soon as the operand has a zero slab 0 on either axis
        c0 = T.new(np.array([[0.0, 0.5], [0.0, 0.5]]).reshape(2, 2, 1), [6, 12])
        R.keep(f"{tag}.c0.linear", c0.extract_linear())
        wc = p.subst_var(1, c0)
        R.probe(f"{tag}.cross_c0", wc, none(wc.coeffs_shape()) if tag == "k2" else slabs(wc.coeffs_shape(), {0: 1}))
        m0 = T.new(np.array([[0.25, 0.0], [0.25, 0.0]]).reshape(2, 1, 2), [6, 12])   # c + [0,0] x_1
        R.keep(f"{tag}.m0.linear", m0.extract_linear())
        r0 = p.subst_var(1, m0)
        mi = T.new(np.array([[0.25, 1.0], [0.25, float("inf")]]).reshape(2, 1, 2), [6, 12])   # c + [1, inf] x_1
        ri = p.subst_var(1, mi)
        zi = none(ri.coeffs_shape())
        if tag == "other_axis":
            zi[0, 0] = True                    # row 0 is [0,0] * m = NaN wherever a power of m arrives: only x_1^0 stays [0,0]
        R.probe(f"{tag}.m_inf", ri, zi)
        z0 = ~slabs(r0.coeffs_shape(), {1: 1})    # every power of m = [0,0] above the 0th is [0,0]: only x_1^0 is left
        R.probe(f"{tag}.m_zero", r0, z0 | slabs(r0.coeffs_shape(), {0: 1}) if tag == "other_axis" else z0)


# ---- consumers at support_proves_nonlinear's edge -------------------------------------------------------------------------------------
@case("consumer_edges", boundary=(("32x2.z1", lambda m: m.shape == (32, 2) and m[:, 0].all() and not m[:, 1].any()), ("22x3.z0", lambda m: m.shape == (22, 3) and not m.any())))
def accumulators_of_two_and_three_coefficients(T, R):
    """Horner accumulators (one slab of the operand) with one axis of 2, two axes of 2, one axis of 3 — with and without a
    leading zero slab: the consumers in Run.finish() go through them."""
    for shape in ((32, 2), (16, 2, 2), (22, 3), (8, 3, 3)):
        for zv in (0, 1):
            Z = slabs(shape, {len(shape) - 1: 1}) if zv else none(shape)
            p = mk(T, shape, 100 + 2 * len(shape) + zv + shape[0], Z if zv else None)
            R.probe(f"{'x'.join(map(str, shape))}.z{zv}", p, Z)
            q = p * T.from_scalar(NZ)
            R.probe(f"{'x'.join(map(str, shape))}.z{zv}.scaled", q, Z)
    # a tensor that IS linear, and one that is all zero, among the consumers
    lin = none((32, 2)) | True
    lin[0, 0] = lin[1, 0] = False
    R.probe("linear", mk(T, (32, 2), 120, lin), lin)
    lin2 = none((32, 2)) | True
    lin2[0, 0] = lin2[0, 1] = False
    R.probe("linear.axis1", mk(T, (32, 2), 121, lin2), lin2)


# ---- memoised verdicts shared between handles [Buf::lin_state / lin_c / lin_m / lin_var, gft_poly::c0_known] ---------------------------
# (f64 and interval.)  A verdict is memoised through one handle and consumed through another handle on the same buffer; every
# answer must be the oracle's for THAT handle.
MEMO_TENSORS = ("linear_x1", "linear_x0", "nonlinear", "nonlinear_outside_the_box", "all_zero", "constant_only")
MEMO_SHAPE, MEMO_DEG = (3, 4, 1), [3, 4, 2]


def _memo_tensor(T, which):
    a = 0.25 + splitmix64_uniform(131, 12).reshape(MEMO_SHAPE)
    keep = {"linear_x1": [(0, 0, 0), (0, 1, 0)], "linear_x0": [(0, 0, 0), (1, 0, 0)], "nonlinear": None,
            "nonlinear_outside_the_box": [(0, 0, 0), (0, 1, 0), (2, 3, 0)], "all_zero": [], "constant_only": [(0, 0, 0)]}[which]
    if keep is not None:
        m = np.zeros(MEMO_SHAPE, dtype=bool)
        for k in keep:
            m[k] = True
        a = np.where(m, a, 0.0)
    if T.WIDTH == 2:
        a = np.stack([a, np.where(a != 0.0, a + 0.125, 0.0)])
    return T.new(a, MEMO_DEG)


MEMO_DERIVED = {
    "clone": lambda T, a: a.clone(),
    "extend_to_dim": lambda T, a: a.extend_to_dim(5, 3),
    "drop_unit_axis": lambda T, a: a.remove_last_variable(),
    "truncated_view": lambda T, a: a.truncate_to_degree_p1(2),
    "minus_constant_term": lambda T, a: a - T.from_scalar(a.constant_term()),
    "scaled": lambda T, a: a * T.from_scalar(0.5),
}


def _ask(R, tag, h):
    R.keep(tag + ".extract_linear", h.extract_linear())
    R.keep(tag + ".constant_term", h.constant_term())
    R.keep(tag + ".is_zero", h.is_zero())
    R.keep(tag + ".extract_constant", h.extract_constant())


def memo_program(which, order):
    def run(T, R):
        big = T.new(planes(MEMO_SHAPE, 132) if T.WIDTH == 2 else planes(MEMO_SHAPE, 132)[0], MEMO_DEG)
        for name, derive in MEMO_DERIVED.items():
            a = _memo_tensor(T, which)
            if order == "a_first":
                _ask(R, f"{name}.a", a)
                d = derive(T, a)
                _ask(R, f"{name}.d", d)
            elif order == "d_first":
                d = derive(T, a)
                _ask(R, f"{name}.d", d)
                _ask(R, f"{name}.a", a)
                _ask(R, f"{name}.d.again", d)
            else:  # the verdict is formed inside subst_var (the substitution's scan) and consumed by the questions afterwards
                d = derive(T, a)
                R.hold(f"{name}.subst_by_d.first", big.subst_var(1, d))
                _ask(R, f"{name}.a", a)
                _ask(R, f"{name}.d", d)
            R.hold(f"{name}.d", d)
            R.hold(f"{name}.subst_by_d", big.subst_var(1, d))   # the substitution's verdict decides the path taken here
            R.hold(f"{name}.subst_by_a", big.subst_var(0, a))
            R.hold(f"{name}.d_times_a", d * a)                  # Mul asks both operands whether they are linear
    run.__name__ = f"memo_{which}_{order}"
    return run


MEMO_ORDERS = ("a_first", "d_first", "subst_first")


# ---- regressions: the minimal programs of the unsound claims this suite found ---------------------------------------------------------
@case("regressions", options=({"defer": 0},), boundary=(("quotient", lambda m: not m.any()),))
def regression_zero_slab_divided_by_zero(T, R):
    """[0,0] / [0,0] is NaN: a gathered quotient by [0,0] kept the source's "leading zero slabs" (the chain rule dropped it)."""
    shape = (6, 12)
    p, Z = measured(T, R, "p", shape, 141, slabs(shape, {0: 1}), v=1)
    R.probe("quotient", p / T.from_scalar(ZERO), none(shape))
    R.probe("row.quotient", p.coefficients_of_term(1, 2) / T.from_scalar(ZERO), none((6, 1)))


@case("regressions", options=({"defer": 0},), boundary=(("horner", lambda m: m[0, 0] and m.sum() == 1),))
def regression_zero_slab_times_an_infinite_bound(T, R):
    """[0,0] * s is NaN when a bound of s is infinite: scalings, scaling tables and Horner loops with such an m kept zero slabs
    that hold NaN.  (An observation at such an x is here as an edge only: observe_chain takes its step-by-step path for a
    non-finite x and claimed nothing, which was sound.)"""
    shape = (6, 12)
    p, Z = measured(T, R, "p", shape, 142, slabs(shape, {0: 1}), v=1)
    zt, zz = zeros_measured(T, R, "zeros", shape)
    s = T.from_scalar(INF)
    R.probe("p*inf", p * s, none(shape))
    R.probe("inf*p", s * p, none(shape))
    R.probe("zeros*inf", zt * s, none(shape))
    R.probe("row*inf", p.coefficients_of_term(0, 0) * s, none((1, 12)))
    m_inf = T.new(np.array([[0.0, 1.0], [0.0, float("inf")]]).reshape(2, 1, 2), [6, 12])      # 0 + [1, inf] x_1
    zs = Z.copy()
    zs[:, 1:] = False                          # slab k of x_1 is multiplied by m^k: NaN in row 0 for k >= 1
    R.probe("scale", p.subst_var(1, m_inf), zs)
    R.probe("zeros.scale", zt.subst_var(1, m_inf), zs | slabs(shape, {1: 1}))
    q, Zq = measured(T, R, "q", shape, 143, slabs(shape, {1: 1}), v=0)
    q2 = q.mul_var(NZ, 1, list(shape), list(shape)) + zt                                       # zero slabs 0 and 1 of x_1
    R.probe("q2", q2, slabs(shape, {1: 2}))
    r = q2.observe_chain(1, INF, [NZ], 12)     # out[0] = x * D[0] with D[0] = [0,0]
    R.probe("observe", r, none(r.coeffs_shape()))
    lin = T.new(np.array([[0.25, 1.0], [0.25, float("inf")]]).reshape(2, 1, 2), [6, 12])     # c + [1, inf] x_1
    h = p.subst_var(1, lin)
    zh = none(h.coeffs_shape())
    zh[0, 0] = True
    R.probe("horner", h, zh)
