"""The references of test_streaming_variants_gpu.py, checked on their own (no GPU): the oracle's `sum_axis` — until now
"recalled, not pinned"  — against exact integer arithmetic and against a correctly rounded sum, at every
length and shape the GPU module uses; and the oracle's `extract_linear` / `==` at the spoiler positions of the scan tests.

This validates the test data (the integer data really is order-independent, the cancellation data really cancels), shows
that the reference alone stays within the order-independent bound, and pins the oracle's fold for len >= 8.
"""
import numpy as np
import pytest

import _streaming_cases as sc


def _run(T, arr, deg, v, n):
    r = T.new(arr, deg).shift_down(v, n)
    return r, np.asarray(r.array())


def check_oracle_shift_down(OTP, OTPI, case, kinds=("int", "cancel")):
    cid, shape, deg, v, n, _ = case
    for seed, kind in enumerate(kinds):
        x = sc.DATA[kind](shape, 7000 + 13 * seed + sum(shape))
        r, got = _run(OTP, x, deg, v, n)
        want_deg = list(deg)
        want_deg[v] = deg[v] - n
        assert r.degrees_p1() == tuple(want_deg), cid
        if kind == "int":
            exact = sc.shift_down_exact(x, v, n)
            assert got.shape == exact.shape, cid
            assert np.array_equal(got, exact.astype(np.float64)), cid
            # order-independence of the data itself: the reversed and the pairwise (numpy) order give the same doubles
            t = sc.summed_terms(x, v, n)
            assert np.array_equal(t[::-1].cumsum(axis=0)[-1], t.sum(axis=0)), cid
            assert np.array_equal(t.sum(axis=0), exact.astype(np.float64).take(0, axis=v).reshape(-1)), cid
            # intervals: every add widens by an ulp (iv:126-139), so the sum encloses the exact value
            iv = np.asarray(_run(OTPI, sc.as_interval(x, point=True), deg, v, n)[1])
            assert np.all(iv[0] <= exact) and np.all(exact <= iv[1]), cid
            S = np.abs(t).sum(axis=0)  # ... by at most an ulp of the running endpoint per side and add
            width0 = (iv[1] - iv[0]).take(0, axis=v).reshape(-1)
            assert np.all(width0 <= 2 * t.shape[0] * np.spacing(S)), cid
        else:
            worst = sc.assert_within_fsum_bound(x, v, n, got, f"oracle {cid}")
            assert worst <= 1.0
            if kind == "cancel":  # the data does cancel: the sums are far smaller than their terms
                t = sc.summed_terms(x, v, n)
                if t.shape[0] >= 64 and v == len(shape) - 1 and t.shape[0] == shape[v]:  # (whole rows: every term has its partner)
                    assert np.median(np.abs(t.sum(axis=0)) / np.abs(t).sum(axis=0)) < 1e-3, cid


@pytest.mark.parametrize("L", sc.WAVE_LENGTHS)
def test_oracle_long_row_sums_exact_and_within_fsum_bound(L, OTP, OTPI):
    for case in sc.wave_cases(L):
        check_oracle_shift_down(OTP, OTPI, case)


@pytest.mark.parametrize("case", sc.WAVE_EXTRA, ids=[c[0] for c in sc.WAVE_EXTRA])
def test_oracle_prefix_and_rank3_row_sums(case, OTP, OTPI):
    check_oracle_shift_down(OTP, OTPI, case)


@pytest.mark.parametrize("L", sc.UNROLL8_LENGTHS)
def test_oracle_fold_of_eight_exact_and_within_fsum_bound(L, OTP, OTPI):
    """ndarray's unrolled_fold as the oracle restates it: main loop (L >= 8), tail, and the (p0+p4)+(p1+p5)+.. combine."""
    for case in sc.unroll8_cases(L):
        check_oracle_shift_down(OTP, OTPI, case)


def test_oracle_slab_by_slab_sums(OTP, OTPI):
    for case in sc.seq_cases():
        check_oracle_shift_down(OTP, OTPI, case)


@pytest.mark.parametrize("case", sc.BIG_SEQ_CASES + [sc.BIG_INTERVAL_CASE], ids=[c[0] for c in sc.BIG_SEQ_CASES] + [sc.BIG_INTERVAL_CASE[0]])
def test_oracle_sums_above_one_grid_pass_exact(case, OTP, OTPI):
    check_oracle_shift_down(OTP, OTPI, case, kinds=("int",))


def test_fsum_bound_rejects_a_dropped_term():
    """The bound is tight enough to see one lost term of cancelling data (what a wrong lane stride does)."""
    x = sc.cancel_data((3, 193), 99)
    good = np.array([[np.sum(r)] for r in x])
    sc.assert_within_fsum_bound(x, 1, 192, good, "numpy")
    bad = good.copy()
    bad[1, 0] -= x[1, 64]
    with pytest.raises(AssertionError):
        sc.assert_within_fsum_bound(x, 1, 192, bad, "dropped")


# ---- the oracle's verdicts at the spoiler positions ----------------------------------------------------------------------
@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_oracle_extract_linear_at_spoiler_positions(interval, OTP, OTPI):
    T = OTPI if interval else OTP
    mk = (lambda a: np.stack([a, a])) if interval else (lambda a: a)
    sv = (lambda x: (x, x)) if interval else (lambda x: x)
    shape, blocks = sc.SCAN_SHAPES[0]
    t = sc.linear_tensor(shape)
    p = T.new(mk(t), shape)
    assert p.extract_linear() == (sv(0.75), sv(-1.5), 0)
    assert not p.is_constant()
    for pos in sc.spoiler_positions(shape, blocks):
        s = t.copy()
        s.flat[pos] = 0.5
        assert T.new(mk(s), shape).extract_linear() is None, pos
    # a coefficient with two non-zero axes, and the interval [0, tiny] (not an exact zero)
    s = t.copy()
    s[1, 1, 0] = 0.5
    assert T.new(mk(s), shape).extract_linear() is None
    if interval:
        s = np.stack([t, t])
        s[1].flat[numel_minus_one(shape)] = 5e-324
        assert T.new(s, shape).extract_linear() is None


def numel_minus_one(shape):
    return sc.numel(shape) - 1


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_oracle_equality_at_single_differences(interval, OTP, OTPI):
    T = OTPI if interval else OTP
    mk = (lambda a: np.stack([a, a + 1.0])) if interval else (lambda a: a)
    x = sc.pos_data(sc.EQ_SHAPE, 4242)
    a = T.new(mk(x), sc.EQ_SHAPE)
    assert a == T.new(mk(x), sc.EQ_SHAPE)
    for pos in sc.EQ_POSITIONS:
        y = x.copy()
        y.flat[pos] = np.nextafter(y.flat[pos], 2.0)
        assert a != T.new(mk(y), sc.EQ_SHAPE), pos
        y = x.copy()
        y.flat[pos] = np.nan  # derived PartialEq: NaN != NaN, so a tensor holding one is not even equal to itself
        b = T.new(mk(y), sc.EQ_SHAPE)
        assert not (b == b) and a != b, pos
