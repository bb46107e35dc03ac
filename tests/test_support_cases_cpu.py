"""The fixed programs of tests/_support_cases.py on the CPU oracle alone: the oracle accepts every step, and the true zero
pattern of every probed step is the one the case states.  This validates the inputs of tests/test_support_claims_gpu.py — a
failure there is then a finding about the library, not an accident of the data — and it settles what `[0,0] / s` is."""
import numpy as np
import pytest

import _support_cases as sc
from _support_model import claim_holds, zero_mask


def _run(case, T):
    R = sc.Run(T)
    case.fn(T, R)                    # raises if the oracle refuses a step: fixed programs, none may be abandoned
    arrays, kept = R.finish()
    return R, arrays, kept


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: f"{c.family}-{c.name}")
def test_true_zero_pattern_is_the_stated_one(case, OTPI):
    R, arrays, _ = _run(case, OTPI)
    assert R.probes, "a case without probes checks nothing"
    for p in R.probes:
        a = arrays[p["name"]][1]
        got = zero_mask(a[0], a[1])
        assert got.shape == p["want"].shape, (case.name, p["name"], got.shape, p["want"].shape)
        bad = np.argwhere(got != p["want"])
        assert len(bad) == 0, (case.name, p["name"], "first mismatch at", tuple(bad[0]), "is zero:", bool(got[tuple(bad[0])]))


def test_every_family_has_a_case_on_its_rules_boundary_and_report(OTP, OTPI, capsys):
    """Per family at least one case names probes whose TRUE zero pattern — the oracle's data, not a flag — sits exactly on the
    rule's edge (shift equals slab, union just touching, pad meets slab, ...); every such predicate must hold."""
    lines = []
    for fam in sc.families():
        cases = [c for c in sc.CASES if c.family == fam]
        probes = on_edge = 0
        for c in cases:
            R, arrays, _ = _run(c, OTPI)
            probes += len(R.probes)
            for name, pred in c.boundary:
                a = arrays[name][1]
                assert pred(zero_mask(a[0], a[1])), (c.name, name, "is not on the boundary it is named for")
            on_edge += 1 if c.boundary else 0
        lines.append(f"support cases: family {fam:18s} cases {len(cases):3d}  probed steps {probes:4d}  boundary cases {on_edge}")
        assert on_edge >= 1, fam
    answers = 0
    for which in sc.MEMO_TENSORS:
        for order in sc.MEMO_ORDERS:
            for T in (OTP, OTPI):
                R = sc.Run(T)
                sc.memo_program(which, order)(T, R)
                answers += len(R.kept) + len(R.held)
    n = len(sc.MEMO_TENSORS) * len(sc.MEMO_ORDERS) * 2
    lines.append(f"support cases: family {'memo':18s} cases {n:3d}  answers and tensors compared {answers} (no zero pattern, no boundary)")
    with capsys.disabled():
        print()
        for ln in lines:
            print(ln)


def test_interval_zero_divided_by_a_scalar(OTPI):
    """What the claims about a division stage rest on: [0,0] / s is [0,0] for every s but [0,0] itself — also for an s that
    merely contains zero — and [0,0] / [0,0] is NaN; a non-zero x / s is never [0,0]."""
    x = np.zeros((2, 1, 2))
    x[:, 0, 1] = (0.5, 0.75)
    p = OTPI.new(x, [1, 2])
    for s, zero_stays in ((sc.NZ, True), (sc.STRADDLE, True), (sc.INF, True), ((-2.0, -1.0), True), (sc.ZERO, False)):
        a = (p / OTPI.from_scalar(s)).array()
        if zero_stays:
            assert a[0, 0, 0] == 0.0 and a[1, 0, 0] == 0.0, (s, a)
        else:
            assert np.isnan(a[0, 0, 0]) and np.isnan(a[1, 0, 0]), (s, a)
        assert not (a[0, 0, 1] == 0.0 and a[1, 0, 1] == 0.0), (s, a)
    # ... and [0,0] * s is [0,0] only for a finite s
    a = (p * OTPI.from_scalar(sc.INF)).array()
    assert np.isnan(a[0, 0, 0]) or np.isnan(a[1, 0, 0]), a


def test_the_model_rejects_wrong_claims():
    """claim_holds on hand-made tensors: each kind accepts its own pattern and names a counter-example for a neighbouring one."""
    z8, h8 = [0] * 8, [0xFFFFFFFF] * 8
    lo = np.ones((4, 5))
    lo[:, 0] = 0.0
    assert claim_holds(3, [0, 1] + [0] * 6, h8, lo, lo) is None
    assert claim_holds(3, [0, 2] + [0] * 6, h8, lo, lo)[0] == (0, 1)
    assert claim_holds(3, [1, 1] + [0] * 6, h8, lo, lo)[0] == (0, 1)
    assert claim_holds(2, z8, h8, lo, lo)[0] == (0, 0)
    assert claim_holds(5, z8, h8, lo, lo)[0] == (0, 1)
    assert claim_holds(4, [0, 1] + [0] * 6, [4, 5] + [0xFFFFFFFF] * 6, lo, lo) is None
    assert claim_holds(4, [0, 1] + [0] * 6, [3, 5] + [0xFFFFFFFF] * 6, lo, lo)[0] == (3, 1)
    assert claim_holds(4, [0, 0] + [0] * 6, [4, 5] + [0xFFFFFFFF] * 6, lo, lo)[0] == (0, 0)
    hi = lo.copy()
    hi[2, 0] = 5e-324                       # [0, 5e-324] is not a zero
    assert claim_holds(3, [0, 1] + [0] * 6, h8, lo, hi)[0] == (2, 0)
    for kind in (0, 1):
        assert claim_holds(kind, z8, h8, lo, hi) is None
    assert claim_holds(3, [0] * 7 + [1], h8, lo, lo)[0] == (0, 1)   # a slab on an axis the tensor does not have: all zero


@pytest.mark.parametrize("interval", [False, True])
@pytest.mark.parametrize("order", sc.MEMO_ORDERS)
@pytest.mark.parametrize("which", sc.MEMO_TENSORS)
def test_memo_programs_run_on_the_oracle(which, order, interval, OTP, OTPI):
    """The memo-sharing programs are accepted step by step, and their tensors are what their names say."""
    T = OTPI if interval else OTP
    R = sc.Run(T)
    sc.memo_program(which, order)(T, R)
    arrays, kept = R.finish()
    answers = dict(kept)
    lin = answers["clone.a.extract_linear"]
    assert (lin is not None) == (which in ("linear_x1", "linear_x0", "all_zero", "constant_only")), (which, lin)
    if which == "linear_x1":
        assert lin[2] == 1
    if which == "nonlinear_outside_the_box":   # the buffer is not linear, its truncated view is
        assert answers["truncated_view.d.extract_linear"] is not None and answers["truncated_view.a.extract_linear"] is None
