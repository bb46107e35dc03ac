"""The interval handle API's zero-pattern proofs, rule by rule, against the data.

Every fixed program of tests/_support_cases.py runs on the GPU without anything being read back in between; after each step the
library's claim for the new handle is read through the test-only `gfti_support_claim` (metadata: nothing is launched) and
checked with tests/_support_model.claim_holds against the ORACLE's tensor for that step.  At the end every probed tensor, and
what the consumers of claims (a proven subst_var, extract_linear) made of it, must be the oracle's bit for bit — with the proofs
on and off, and with the recording switches the family names.  Soundness is required, completeness is not: "unknown" where a
claim would have been possible never fails; that the claims have not all turned into "unknown" is asserted per family."""
import ctypes as C
import os

import numpy as np
import pytest

import _support_cases as sc
from _support_model import INFORMATIVE, claim_holds, proves_nonlinear

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle_run(key, fn, T):
    """The oracle's run of a program: computed once, shared, never changed."""
    if key not in _ORACLE:
        R = sc.Run(T)
        fn(T, R)
        lin = [p["h"].extract_linear() for p in R.probes]
        arrays, kept = R.finish()
        _ORACLE[key] = (R.probes, lin, arrays, kept)
    return _ORACLE[key]


def _reader(prefix="gfti_"):
    import genfer_amd

    f = getattr(genfer_amd.lib(), prefix + "support_claim")
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def read(h):
        kind, lin, z, hh = C.c_size_t(), C.c_size_t(), (C.c_size_t * 8)(), (C.c_size_t * 8)()
        assert f(h._h, C.byref(kind), z, hh, C.byref(lin)) == 0
        return {"kind": int(kind.value), "z": [int(v) for v in z], "h": [int(v) for v in hh], "lin_state": int(lin.value)}
    return read


def _settle_backoff(G, read):
    """nz_query does not ask for a while after it has met irregular zeros: its process-wide `skip` / `backoff` counters
    (Ops::nz_query, gft_ops_observe.inc) leave at most 256 candidates unasked.  Use that up on throw-away tensors, so that what
    a case measures does not depend on the cases before it: every pass below is one candidate, so the tensor is measured
    after at most 257 of them — 600 leaves room for the cap to double once before this loop has to change."""
    for _ in range(600):
        p = sc.mk(G, (8, 8), 999)
        sc.measure(G, p, 0)
        if read(p)["kind"] == 2:
            return
    raise AssertionError("a tensor without zeros is never measured as such")


# The switches the cases run under and the environment variable that sets each at start-up (gft_init): the library has no
# getter, so "the value before" is the environment's, or the default (on).
_SWITCH_ENV = {"nz_proofs": "GFT_NZ_PROOFS", "lazy_sum": "GFT_LAZY_SUM", "lazy_horner": "GFT_LAZY_HORNER", "batch_dag": "GFT_BATCH",
               "lazy_observe": "GFT_LAZY_OBSERVE", "defer": "GFT_DEFER"}


def _value_before(option):
    v = os.environ.get(_SWITCH_ENV[option])
    return 1.0 if v is None else float(int(v) != 0)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _same_answer(a, b):
    if a is None or b is None or isinstance(a, bool):
        return a == b
    fa = np.array([x for t in (a if isinstance(a, tuple) else (a,)) for x in (t if isinstance(t, tuple) else (t,))], dtype=float)
    fb = np.array([x for t in (b if isinstance(b, tuple) else (b,)) for x in (t if isinstance(t, tuple) else (t,))], dtype=float)
    return _same(fa, fb)


def _gpu_run(key, fn, O, G, read, opts, stats=None):
    """One GPU run of a program under `opts`, checked against the oracle's run; returns the arrays and the claims' kinds."""
    import genfer_amd

    L = genfer_amd.lib()
    oprobes, olin, oarrays, okept = _oracle_run(key, fn, O)
    proofs_on = opts.get("nz_proofs", _value_before("nz_proofs")) != 0
    if read is not None and proofs_on:
        _settle_backoff(G, read)
    try:
        for k, v in opts.items():
            assert L.gft_set_option(k.encode(), float(v)) == 0
        before = genfer_amd.op_stats()
        R = sc.Run(G, read)
        fn(G, R)                                      # nothing is read back: claims are metadata
        assert [p["name"] for p in R.probes] == [p["name"] for p in oprobes]
        arrays, kept = R.finish()
        after = genfer_amd.op_stats()
    finally:
        for k in opts:
            L.gft_set_option(k.encode(), _value_before(k))
    kinds = []
    for p, lin in zip(R.probes, olin):
        want = oarrays[p["name"]][1]
        for when in ("claim", "claim_after"):
            c = p.get(when)
            if c is None:
                continue
            kinds.append(c["kind"])
            bad = claim_holds(c["kind"], c["z"], c["h"], want[0], want[1])
            assert bad is None, (key, opts, p["name"], when, c, bad)
            if proves_nonlinear(c["kind"], c["z"], want[0].shape) and want[0].size >= 3:  # what a consumer concludes
                assert lin is None, (key, opts, p["name"], when, c, "proven not linear, but the oracle extracts", lin)
    assert set(arrays) == set(oarrays)
    for name, (deg, a) in arrays.items():
        odeg, oa = oarrays[name]
        assert deg == odeg and a.shape == oa.shape, (key, opts, name, deg, odeg, a.shape, oa.shape)
        ok = (a == oa) | (np.isnan(a) & np.isnan(oa))
        assert np.all(ok), (key, opts, name, np.argwhere(~ok)[:3].tolist(), a[~ok][:3], oa[~ok][:3])
    assert [n for n, _ in kept] == [n for n, _ in okept]
    for (name, got), (_, want) in zip(kept, okept):
        assert _same_answer(got, want), (key, opts, name, got, want)
    if stats is not None:
        for k in ("scans_proven", "linear_scans", "launches"):
            stats[k] = stats.get(k, 0) + after[k] - before[k]
    return arrays, kinds


def _option_sets(case):
    sets = [{}] + [dict(o) for o in case.options]
    if case.proofs:
        sets += [dict(o, nz_proofs=0) for o in list(sets)]
    return sets


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: f"{c.family}-{c.name}")
def test_claims_hold_for_the_oracles_data(case, OTPI, GTPI):
    read = _reader()
    results = {}
    for opts in _option_sets(case):
        results[tuple(sorted(opts.items()))], _ = _gpu_run(case.name, case.fn, OTPI, GTPI, read, opts)
    ref = results[()]
    for key, arrays in results.items():       # proofs on / off, every switch: the same bits
        for name in ref:
            assert _same(arrays[name][1], ref[name][1]), (case.name, key, name)


@pytest.mark.parametrize("family", sc.families())
def test_family_carries_informative_claims(family, OTPI, GTPI):
    """With default options: some probed step of the family carried a claim of kind 2, 3, 4 or 5, and the proofs answered
    linearity scans — a change that quietly turns every claim into "unknown" fails here instead of passing vacuously."""
    read = _reader()
    kinds, stats = [], {}
    for case in (c for c in sc.CASES if c.family == family):
        _, k = _gpu_run(case.name, case.fn, OTPI, GTPI, read, {}, stats)
        kinds += k
    print(f"support claims: family {family}: kinds {sorted(set(kinds))}, counters {stats}")
    if any(os.environ.get(e) for e in _SWITCH_ENV.values()):
        return  # (a run of the suite under one of the switches checks the bits above only, as test_horner_shapes_gpu does)
    assert any(k in INFORMATIVE for k in kinds), (family, sorted(set(kinds)))
    assert stats["scans_proven"] > 0, (family, stats)


@pytest.mark.parametrize("interval", [False, True])
@pytest.mark.parametrize("order", sc.MEMO_ORDERS)
@pytest.mark.parametrize("which", sc.MEMO_TENSORS)
def test_memoised_verdicts_through_other_handles(which, order, interval, OTP, GTP, OTPI, GTPI):
    """extract_linear / constant_term / is_zero through one handle, then (or before) through a clone, an extended handle, one
    with a trailing unit axis dropped, a truncated view and `p - constant_term(p)` on the same buffer: every answer, and every
    substitution and product that consumes a memoised verdict, is the oracle's for that handle."""
    O, G = (OTPI, GTPI) if interval else (OTP, GTP)
    fn = sc.memo_program(which, order)
    _gpu_run((fn.__name__, interval), fn, O, G, None, {})


def test_f64_handles_claim_nothing(GTP):
    read = _reader("gft_")
    p = GTP.new(sc.planes((6, 12), 7)[0], [6, 12])
    c = read(p)
    assert c["kind"] == 0 and c["lin_state"] == 0, c
    assert p.extract_linear() is None
    assert read(p)["lin_state"] == 1 and read(p.clone())["lin_state"] == 1   # the verdict is the buffer's
