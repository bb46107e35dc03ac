"""The cases of tests/_recur_edge_cases.py are not vacuous: on the ORACLE alone (no GPU) every case shows the features it exists
for — a growth case leaves the exponent window upwards in the middle of a row (or at a later slab), overflows and goes on as
NaN; a decay case passes through normal values below the window, denormals, +0 and -0; the divisor sweep's quotients are
independent and equal numpy's x / d.  These are conditions on the INPUTS: a case that misses one gets another exponent b, never
a weaker probe.  The table's family labels are checked against plan_wavefront (tests/wavefront_plan_check.cpp --family)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _recur_edge_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# Interval planes: the reference's interval arithmetic rounds outwards, so a lower bound never rounds to an exact zero (it stops
# at the smallest denormal) and an overflowed bound stays infinite (inf - inf is widened to an infinite bound, never NaN).  The
# probes that ask for a zero or a NaN therefore hold for the f64 result only; everything else is asked of the `lo` plane too.
def growth_probes(a, ax, what, interval=False):
    c = rc.classify(a)
    for k in ("in_window", "above", "inf") + (() if interval else ("nan",)):
        assert c[k].any(), f"{what}: no {k} coefficient"
    out = np.argwhere(~c["in_window"])
    first = int(out[:, ax].min())
    assert first >= 8, f"{what}: leaves the window at index {first} of axis {ax}, among the first 8"
    if ax == 0 and a.ndim > 1:
        assert not (~c["in_window"][0]).any(), f"{what}: slab 0 already holds a coefficient outside the window"


def decay_probes(a, what, interval=False):
    c = rc.classify(a)
    for k in ("in_window", "below", "denormal") + (() if interval else ("pos_zero", "neg_zero")):
        assert c[k].any(), f"{what}: no {k} coefficient"
    for k in ("inf", "nan", "above"):
        assert not c[k].any(), f"{what}: a {k} coefficient in a decaying quotient"
    first = int(np.flatnonzero(~c["in_window"].reshape(-1))[0])
    assert first >= 8, f"{what}: leaves the window at coefficient {first}, among the first 8"


@pytest.mark.parametrize("row,fam,ax,var,xs,ys", rc.CASES, ids=rc.CASE_IDS)
def test_division_cases_cross_the_switches_on_the_oracle(row, fam, ax, var, xs, ys, OTP, OTPI):
    x, y = rc.operands(row, fam, ax, xs, ys)
    deg = list(row.shape)
    cid = rc.case_id(row, fam, ax, var)
    a, _, stored = rc.oracle_div(OTP, cid, x, y, deg)
    assert tuple(stored) == row.shape
    (growth_probes(a, ax, cid) if fam == "growth" else decay_probes(a, cid))
    for kind, widen in rc.interval_kinds(row, var):
        ai, _, _ = rc.oracle_div(OTPI, (cid, kind), widen(x), widen(y), deg)
        (growth_probes(ai[0], ax, f"{cid} {kind} lo", True) if fam == "growth" else decay_probes(ai[0], f"{cid} {kind} lo", True))


LOG_ROWS = [r for r in rc.TABLE if r.log]


def log_probes(a, name, what, interval=False):
    """as for the quotients: the growth argument's logarithm leaves the window upwards at index 8 or later of the last axis and
    overflows; the decaying arguments' logarithms leave it downwards, not among the first 8 coefficients"""
    c = rc.classify(a)
    if name == "growth":
        for k in ("in_window", "above", "inf") + (() if interval else ("nan",)):
            assert c[k].any(), f"{what}: no {k} coefficient"
        first = int(np.argwhere(~c["in_window"])[:, -1].min())
    else:
        for k in ("in_window", "below", "denormal") + (() if interval else ("pos_zero", "neg_zero")):
            assert c[k].any(), f"{what}: no {k} coefficient"
        first = int(np.flatnonzero(~c["in_window"].reshape(-1))[0])
    assert first >= 8, f"{what}: leaves the window at index {first}, among the first 8"


@pytest.mark.parametrize("row", LOG_ROWS, ids=[r.id for r in LOG_ROWS])
def test_log_and_exp_cases_cross_the_switches_on_the_oracle(row, OTP, OTPI):
    """log of the decaying argument: values below the window, denormals and zeros of both signs; log of (1 - t)(1 - g t): the
    recurrence overflows.  exp of the decaying argument likewise (reference order).  Interval results: the `lo` plane."""
    deg = list(row.shape)
    for name, arg in rc.log_arguments(row):
        a, _, _ = rc.oracle_unary(OTP, (row.id, name, "f64"), "log", arg, deg)
        log_probes(a, name, f"log {row.id} {name}")
        for kind, widen in rc.interval_kinds(row):
            ai, _, _ = rc.oracle_unary(OTPI, (row.id, name, f"interval_{kind}"), "log", widen(arg), deg)
            log_probes(ai[0], name, f"log {row.id} {name} {kind} lo", True)
    if row.exp:
        arg = rc.decay(row.shape)[1]
        a, _, _ = rc.oracle_unary(OTP, (row.id, "decay", "f64"), "exp", arg, deg)
        planes = [(a, "f64")]
        for kind, widen in rc.interval_kinds(row):
            planes.append((rc.oracle_unary(OTPI, (row.id, "decay", f"interval_{kind}"), "exp", widen(arg), deg)[0][0], f"{kind} lo"))
        for a, what in planes:
            c = rc.classify(a)
            # (an exponential's coefficient is a sum formed from +0 divided by k: its exact zeros are +0 unless every term is -0;
            # an interval's lower bound rounds outwards and stops at the smallest denormal)
            for k in ("in_window", "below", "denormal") + (("pos_zero",) if what == "f64" else ()):
                assert c[k].any(), f"exp {row.id} {what}: no {k} coefficient"
            first = int(np.flatnonzero(~c["in_window"].reshape(-1))[0])
            assert first >= 8, f"exp {row.id} {what}: leaves the window at coefficient {first}, among the first 8"


@pytest.mark.parametrize("shape,reduced", rc.SWEEP_SHAPES, ids=["x".join(map(str, s)) for s, _ in rc.SWEEP_SHAPES])
def test_sweep_quotients_are_independent_and_equal_numpy(shape, reduced, OTP):
    """coefficients 0 .. n - 2 of x / y, y = (d, 0, .., 0, 0.5), are x[c] / d: the oracle and numpy agree bit for bit, the
    divisor stays stored at its full length, and the numerators cover every side of the window for divisors on every side"""
    seen = {k: 0 for k in ("in_window", "above", "below", "denormal")}
    for i, d in enumerate(rc.sweep_divisors(reduced)):
        x, y, valid = rc.divisor_sweep(shape, float(d), seed=2501 + 7 * i)
        a, _, stored = rc.oracle_div(OTP, ("sweep", shape, i), x, y, list(shape))
        assert tuple(stored) == tuple(shape)
        with np.errstate(under="ignore"):
            want = x / d
        msg = rc.describe_mismatch(f"sweep {shape} d = {float(d)!r} (oracle against numpy)", want[valid], a[valid])
        assert msg is None, msg
        c = rc.classify(x[valid])
        for k in seen:
            seen[k] += int(c[k].sum())
    assert all(seen.values()), seen


def test_negative_zero_rows_case_has_whole_rows_of_negative_zero(OTP):
    x, y = rc.negative_zero_rows()
    a, _, stored = rc.oracle_div(OTP, "negative_zero_rows", x, y, list(y.shape))
    assert tuple(stored) == y.shape
    c = rc.classify(a)
    assert c["in_window"][:2].all() and c["neg_zero"][2].all() and c["neg_zero"][3, :-1].all() and a[3, -1] != 0.0


def test_sweep_divisors_cover_both_sides_of_the_window():
    d = rc.sweep_divisors()
    e = rc.biased_exponent(d)
    assert d.size >= 5 * 66 and (d > 0).sum() >= 32 * 5 and (d < 0).sum() >= 32 * 5
    # fd_mid: 724 .. 1322 pass.  2^-300 * [1, 2) has biased exponent 723 (outside), 2^-299: 724 (inside); 2^299: 1322, 2^300: 1323
    for be, n in ((723, 66), (724, 66), (1322, 66), (1323, 66), (1023, 66)):
        assert (e == be).sum() == n, (be, int((e == be).sum()))
    assert np.nextafter(1.0, 2.0) in d and np.nextafter(2.0, 1.0) in d


def test_table_family_labels_match_the_planner():
    """every wavefront row of the table gets the family it names from plan_wavefront (division, f64, full operands); the rows
    that name none get none"""
    lines = []
    for r in rc.TABLE:
        s = " ".join(str(v) for v in r.shape)
        lines.append(f"0 1 {len(r.shape)} {s} {s} {s}")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "wavefront_plan_check")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genfer_amd", "csrc"),
                               os.path.join(ROOT, "tests", "wavefront_plan_check.cpp"), "-o", exe])
        r = subprocess.run([exe, "--family"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.split()
    assert len(got) == len(rc.TABLE)
    for row, fam in zip(rc.TABLE, got):
        assert fam == (row.family or "none"), (row.kernel, row.shape, fam)
    # the log of the fused-slab-step row takes the row wavefront unless it is switched off (the test switches it off)
    assert {r.family for r in rc.TABLE} >= {"row", "row_q8", "row_q16", "rows_2d", "seg", None}
