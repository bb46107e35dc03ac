"""Random shared-handle programs for the deferred launch graph, as plain data.

A PROGRAM is a dict {"seed", "n", "width", "instrs", "handles"}: `instrs` is a list of instructions over numbered handles,
`handles[k]` the stored shape and degrees the oracle reported for handle k when the program was generated.  The first three
instructions are dense leaves; every other instruction is one of the ten KINDS below — the shapes of use that make recordings
in the library (tests/test_horner_shapes_gpu.py: `_if_statement`, test_launch_graph_batches_bit_exact,
test_recorded_sums_nested_add_bit_exact) — applied to handles drawn from ALL earlier ones, so most handles have several
consumers, on different levels of the graph.  `fan` repeats an instruction with other scalars on the same inputs (what the
evaluator does for the input points of one depth): several items of one geometry in one level.

A SCHEDULE says when values are read and when handles are released; `plan` turns (program, schedule) into a list of actions
that depends on the seed only, `replay` executes it on any bound TaylorPoly class (oracle or product, f64 or interval) and
returns what it read.  The generator runs the oracle to learn shapes (an instruction whose result would stay on the host
tier is discarded), nothing here touches the product: this module imports neither torch nor genfer_amd.lib().
"""
import random

import numpy as np

from conftest import splitmix64_uniform

LEAF_N = 64
N_LEAVES = 3
# HOST_MAX_ELEMS_DEFAULT of the library: a tensor of this many coefficients or fewer stays on the host tier under the default
# dispatch and nothing is recorded for it
SIZE_FLOOR = 2048
KINDS = ("obs", "obs_scaled", "obs_add", "sum", "mul_linear", "addsub", "subst", "add_scaled", "derive_scale", "scale")
OBS_X = (0.9, 0.3, 0.7, 1.0, 0.0)
SUBST_X = (0.9, 0.8, 0.25, 0.0)
FANS = (1, 1, 1, 2, 5)
SCHEDULES = ("last_first", "as_created", "interleaved", "drops", "grow")
READERS = ("array", "constant_term", "coefficient", "is_zero", "clone_array")


# ---- one instruction on one class ------------------------------------------------------------------------------------------
def _leaf_array(seed, n, width):
    base = (0.05 + 0.95 * splitmix64_uniform(seed, n * n)).reshape(n, n)
    return np.stack([base, base * (1 + 1e-15)]) if width == 2 else base


def _execute(T, H, ins):
    """Creates ins["outs"] in the dict H.  Temporaries die with their expressions; nothing but H keeps a handle."""
    sc = (lambda x: (x, x)) if T.WIDTH == 2 else (lambda x: x)
    S = lambda x: T.from_scalar(sc(x))
    kind = ins["kind"]
    if kind == "leaf":
        n = ins["n"]
        H[ins["outs"][0]] = T.new(_leaf_array(ins["seed"], n, T.WIDTH), [n, n])
        return
    i = ins["ins"]
    for out, p in zip(ins["outs"], ins["params"]):
        if kind == "obs":
            H[out] = H[i[0]].observe_chain(p["v"], sc(p["x"]), [sc(c) for c in p["cs"]], p["d"])
        elif kind == "obs_scaled":
            H[out] = (H[i[0]] * S(p["s"])).observe_chain(p["v"], sc(p["x"]), [sc(c) for c in p["cs"]], p["d"])
        elif kind == "obs_add":
            l = H[i[0]].observe_chain(p["v"], sc(p["x"]), [sc(c) for c in p["cs"]], p["d"]) * S(p["s1"])
            r = H[i[1]].observe_chain(p["v2"], sc(p["x2"]), [sc(c) for c in p["cs2"]], p["d"]) * S(p["s2"])
            H[out] = (l - r) if p["sub"] else (l + r)
            del l, r
        elif kind == "sum":
            l, r = H[i[0]] * S(p["s1"]), H[i[1]] * S(p["s2"])
            H[out] = (l - r) if p["sub"] else (l + r)
            del l, r
        elif kind == "mul_linear":
            lin1 = T.var_with_degrees_p1(p["v"], sc(0.0), p["deg"]) * S(p["m1"]) + S(p["c1"])
            lin2 = T.var_with_degrees_p1(p["v"], sc(0.0), p["deg"]) * S(p["m2"]) + S(p["c2"])
            H[out] = H[i[0]] * lin1 + H[i[1]] * lin2
            del lin1, lin2
        elif kind == "addsub":
            H[out] = (H[i[0]] - H[i[1]]) if p["sub"] else (H[i[0]] + H[i[1]])
        elif kind == "subst":
            # the interpreter's Subst arm: subst - constant_term(subst) (for intervals a few-ulp constant is left)
            sub = T.var_with_degrees_p1(p["v"], sc(p["x"]), p["deg"]) * S(p["m"])
            sub = sub - T.from_scalar(sub.constant_term())
            H[out] = H[i[0]].subst_var(p["v"], sub)
            del sub
        elif kind == "add_scaled":
            H[out] = H[i[0]].add_scaled(H[i[1]], sc(p["c"]))
        elif kind == "derive_scale":
            H[out] = H[i[0]].derive_scale(p["v"], sc(p["c"]), p["d"])
        elif kind == "scale":
            H[out] = H[i[0]] * S(p["s"])
        else:
            raise ValueError(kind)


# ---- the generator ---------------------------------------------------------------------------------------------------------
def _scalar(rng, lo=0.1, hi=1.2):
    return round(rng.uniform(lo, hi), 4)


def _params(rng, kind, degs, k):
    """The scalars of repeat k of one instruction; `degs` are the degrees of its operands (the oracle's)."""
    dmin = min(min(d) for d in degs)
    cs = lambda n: [round(rng.uniform(0.05, 0.4), 4) for _ in range(n)]
    if kind in ("obs", "obs_scaled"):
        n = rng.randint(1, 3)
        p = {"v": rng.randrange(2), "x": OBS_X[(rng.randrange(5) + k) % 5], "cs": cs(n), "d": dmin - n}
        if kind == "obs_scaled":
            p["s"] = _scalar(rng)
        return p
    if kind == "obs_add":
        n1, n2 = rng.randint(1, 3), rng.randint(1, 3)
        return {"v": rng.randrange(2), "x": OBS_X[(rng.randrange(5) + k) % 5], "cs": cs(n1), "v2": rng.randrange(2), "x2": OBS_X[rng.randrange(5)],
                "cs2": cs(n2), "d": dmin - max(n1, n2), "s1": _scalar(rng), "s2": _scalar(rng), "sub": rng.random() < 0.3}
    if kind == "sum":
        return {"s1": _scalar(rng), "s2": _scalar(rng), "sub": rng.random() < 0.5}
    if kind == "mul_linear":
        m1, m2 = round(rng.uniform(0.1, 0.9), 4), round(rng.uniform(0.1, 0.9), 4)
        return {"v": rng.randrange(2), "deg": [dmin, dmin], "m1": m1, "c1": round(1 - m1, 4), "m2": m2, "c2": round(1 - m2, 4)}
    if kind == "addsub":
        return {"sub": rng.random() < 0.5}
    if kind == "subst":
        return {"v": rng.randrange(2), "x": SUBST_X[rng.randrange(4)], "deg": list(degs[0]), "m": round(rng.uniform(0.6, 1.0), 6)}
    if kind == "add_scaled":
        return {"c": _scalar(rng, 0.2, 1.5)}
    if kind == "derive_scale":
        return {"v": rng.randrange(2), "c": _scalar(rng), "d": dmin - 1}
    if kind == "scale":
        return {"s": _scalar(rng, 0.2, 1.5)}
    raise ValueError(kind)


ARITY = {"obs": 1, "obs_scaled": 1, "obs_add": 2, "sum": 2, "mul_linear": 2, "addsub": 2, "subst": 1, "add_scaled": 2, "derive_scale": 1, "scale": 1}


def _pick(rng, nh, used):
    """An operand among the nh earlier handles: mostly one of the last eight or, more often than not, one
    of the last sixteen that already has exactly one consumer — so most handles end up shared, by instructions recorded at different times."""
    if rng.random() < 0.7:
        window = range(max(0, nh - 8), nh)
        once = [h for h in range(max(0, nh - 16), nh) if used.get(h, 0) == 1]
        if once and rng.random() < 0.6:
            return once[rng.randrange(len(once))]
        return window[rng.randrange(len(window))]
    return rng.randrange(nh)


def generate(T, seed, n_instr=40, n=LEAF_N):
    """A program of `n_instr` instructions behind three leaves.  T is the ORACLE's class of the element type the program is
    for: every candidate runs on it, its shapes are kept, and a candidate whose result would store SIZE_FLOOR coefficients
    or fewer is discarded (another operand choice of the same kind is drawn).  The oracle must not refuse anything: its
    error is not caught."""
    rng = random.Random(seed)
    H, instrs, handles = {}, [], []

    def accept(ins):
        instrs.append(ins)
        for out in ins["outs"]:
            handles.append({"shape": tuple(H[out].coeffs_shape()), "deg": tuple(H[out].degrees_p1())})

    for k in range(N_LEAVES):
        ins = {"kind": "leaf", "ins": [], "outs": [k], "fan": 1, "n": n, "seed": seed * 1000 + k}
        _execute(T, H, ins)
        accept(ins)
    deck, discarded, used = [], 0, {}
    while len(instrs) < N_LEAVES + n_instr:
        if not deck:  # every ten instructions use every kind once
            deck = list(KINDS)
            rng.shuffle(deck)
        kind = deck.pop()
        for _attempt in range(50):
            nh = len(handles)
            ops = [_pick(rng, nh, used) for _ in range(ARITY[kind])]
            fan = FANS[rng.randrange(len(FANS))]
            degs = [handles[h]["deg"] for h in ops]
            ins = {"kind": kind, "ins": ops, "outs": list(range(nh, nh + fan)), "fan": fan,
                   "params": [_params(rng, kind, degs, k) for k in range(fan)]}
            if any(p.get("d", 1) < 1 for p in ins["params"]):
                discarded += 1
                continue
            _execute(T, H, ins)
            if all(int(np.prod(H[out].coeffs_shape())) > SIZE_FLOOR for out in ins["outs"]):
                accept(ins)
                for h in set(ops):
                    used[h] = used.get(h, 0) + 1
                break
            for out in ins["outs"]:
                del H[out]
            discarded += 1
    H.clear()
    return {"seed": seed, "n": n, "width": T.WIDTH, "instrs": instrs, "handles": handles, "discarded": discarded}


def consumers(program):
    """handle -> indices of the instructions that read it (each instruction once)"""
    use = {k: [] for k in range(len(program["handles"]))}
    for idx, ins in enumerate(program["instrs"]):
        for h in sorted(set(ins["ins"])):
            use[h].append(idx)
    return use


# ---- schedules -------------------------------------------------------------------------------------------------------------
def plan(program, schedule):
    """The actions of one replay: ("exec", instruction index), ("read", handle, reader, index or None), ("release", handle).
    Random choices come from the program's seed and the schedule's name alone."""
    instrs, handles = program["instrs"], program["handles"]
    rng = random.Random(program["seed"] * 7919 + sum(map(ord, schedule)))
    every = list(range(len(handles)))
    acts = []
    rd = lambda h, reader="array", idx=None: ("read", h, reader, idx)
    shuffled = lambda seq: rng.sample(list(seq), len(seq))
    if schedule == "straight":  # the reference order: everything recorded, every handle read in creation order
        acts = [("exec", i) for i in range(len(instrs))] + [rd(h) for h in every]
    elif schedule == "last_first":
        acts = [("exec", i) for i in range(len(instrs))] + [rd(h) for h in reversed(every)]
    elif schedule == "as_created":
        for i, ins in enumerate(instrs):
            acts.append(("exec", i))
            acts += [rd(h) for h in ins["outs"]]
    elif schedule == "interleaved":
        live = 0
        for i, ins in enumerate(instrs):
            acts.append(("exec", i))
            live += len(ins["outs"])
            if rng.random() < 0.2:
                h = rng.randrange(live)
                reader = READERS[rng.randrange(len(READERS))]
                idx = tuple(rng.randrange(s) for s in handles[h]["shape"]) if reader == "coefficient" else None
                acts.append(rd(h, reader, idx))
        acts += [rd(h) for h in shuffled(every)]
    elif schedule == "drops":
        use = consumers(program)
        gone = set()
        for i, ins in enumerate(instrs):
            acts.append(("exec", i))
            for h in sorted(set(ins["ins"])):  # the last consumer of h has been recorded: h may go
                if use[h][-1] == i and rng.random() < 0.5:
                    acts.append(("release", h))
                    gone.add(h)
            for h in ins["outs"]:  # a quarter of the sinks are never read: their recordings must never be needed
                if not use[h] and rng.random() < 0.25:
                    acts.append(("release", h))
                    gone.add(h)
        acts += [rd(h) for h in shuffled([h for h in every if h not in gone])]
    elif schedule == "grow":
        half = N_LEAVES + (len(instrs) - N_LEAVES) // 2
        acts = [("exec", i) for i in range(half)]
        made = sum(len(ins["outs"]) for ins in instrs[:half])
        first = shuffled(range(made))[: made // 3]
        acts += [rd(h) for h in first]
        acts += [("exec", i) for i in range(half, len(instrs))]  # consumers of launched and of still-recorded inputs
        acts += [rd(h) for h in every if h not in set(first)]
    else:
        raise ValueError(schedule)
    return acts


def _read(t, reader, idx):
    if reader == "array":
        return (tuple(t.coeffs_shape()), tuple(t.degrees_p1()), t.array())
    if reader == "clone_array":
        c = t.clone()
        return (tuple(c.coeffs_shape()), tuple(c.degrees_p1()), c.array())
    if reader == "constant_term":
        return np.atleast_1d(np.asarray(t.constant_term(), dtype=np.float64))
    if reader == "coefficient":
        return np.atleast_1d(np.asarray(t.coefficient(idx), dtype=np.float64))
    if reader == "is_zero":
        return bool(t.is_zero())
    raise ValueError(reader)


def replay(T, program, schedule):
    """Runs the program on T under the schedule.  The handles live in ONE dict and nowhere else, so a release frees the
    handle where the plan says.  Returns {(handle, reader): [values in reading order]}."""
    H, out = {}, {}
    for act in plan(program, schedule):
        if act[0] == "exec":
            _execute(T, H, program["instrs"][act[1]])
        elif act[0] == "read":
            out.setdefault((act[1], act[2]), []).append(_read(H[act[1]], act[2], act[3]))
        else:
            del H[act[1]]
    H.clear()
    return out


# ---- comparison ------------------------------------------------------------------------------------------------------------
def same_floats(a, b):
    """bit for bit, a NaN for a NaN (the rule of test_fuzz_gpu._check)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def same_value(want, got):
    if isinstance(want, bool):
        return isinstance(got, bool) and want == got
    if isinstance(want, tuple):
        return want[0] == got[0] and want[1] == got[1] and same_floats(want[2], got[2])
    return same_floats(want, got)


def assert_same_reads(want, got, what=""):
    assert sorted(want) == sorted(got), (what, sorted(set(want) ^ set(got)))
    for key in sorted(want):
        assert len(want[key]) == len(got[key]), (what, key)
        for w, g in zip(want[key], got[key]):
            if not same_value(w, g):
                detail = (w[0], g[0], w[1], g[1]) if isinstance(w, tuple) else (w, g)
                if isinstance(w, tuple) and w[0] == g[0]:
                    bad = ~((w[2] == g[2]) | (np.isnan(w[2]) & np.isnan(g[2])))
                    detail = (int(bad.sum()), w[2][bad][:4], g[2][bad][:4])
                raise AssertionError(f"{what}: handle {key[0]} read by {key[1]} differs from the oracle: {detail}")
