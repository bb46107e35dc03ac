"""The ordered model of the rank-2 exp recurrence (_exp_order_model.py) against the oracle, on the CPU.

The `rev` kernels (exp in arrival order, gft_div2d.hip) are held to the DESCENDING model's bits on the device
(test_exp_arrival_order_gpu.py).  That only means something if the model is right and the data can tell the two orders apart: here the ASCENDING model must be the
oracle's bits for every shape, the descending one must differ from it somewhere, and their distance must respect the
project's 1e-10 contract (shown for the reference's arithmetic alone, no kernel involved)."""
import numpy as np
import pytest

from _exp_order_model import ALL_CASES, NW, WAVEFRONT_FAMILIES, TILED_MIN_MACS_DEFAULT, SWITCH_ABOVE, SWITCH_BELOW, batch_rows, case_data, criterion, exp_model, planned

IDS = [c.id for c in ALL_CASES]


@pytest.mark.parametrize("cid", IDS)
def test_ascending_model_is_the_oracle(cid):
    d = case_data(cid)
    assert d.asc.shape == d.want.shape
    assert np.array_equal(d.asc, d.want, equal_nan=True), np.argwhere(~((d.asc == d.want) | (np.isnan(d.asc) & np.isnan(d.want))))[:5]


@pytest.mark.parametrize("cid", [c.id for c in ALL_CASES if c.special in (None, "wide")])
def test_the_data_tells_the_orders_apart(cid):
    """Rows with three or more source rows exist in every case (k0 >= 3 with xn0 >= 4), and mixed-sign data makes their sums
    order-dependent: a kernel that ignored `rev`, or reversed the wrong range, cannot pass the descending comparison."""
    d = case_data(cid)
    differ = d.desc != d.asc
    assert differ.any()
    assert not differ[:3].any()  # rows 0 .. 2 have at most two source rows: the order cannot matter there
    if d.case.family in WAVEFRONT_FAMILIES and d.want.shape[0] > 4:
        assert differ[4:].any(axis=1).mean() > 0.5, "most rows should discriminate"


@pytest.mark.parametrize("cid", [c.id for c in ALL_CASES if c.special in (None, "wide")])
def test_descending_order_is_within_the_contract(cid):
    d = case_data(cid)
    assert np.all(np.isfinite(d.bound))
    err = np.abs(d.desc - d.asc)
    assert np.all(err <= 1e-10 * d.bound), (err / d.bound).max()


def test_result_shapes():
    """The oracle's result has the requested extents — except where the argument's rows have one coefficient: then the
    result's rows have one too (mt:406-417) and the exponential is a line."""
    for c in ALL_CASES:
        d = case_data(c.id)
        assert d.want.shape == ((c.n[0], 1) if c.family == "line" else c.n), c.id
        assert tuple(d.degrees_p1) == c.n


def test_wide_case_reaches_1e100():
    for c in ALL_CASES:
        if c.special == "wide":
            d = case_data(c.id)
            assert np.abs(d.want[0]).max() >= 1e100 and np.all(np.isfinite(d.want))


def test_switch_point_brackets_the_default_threshold():
    assert criterion(SWITCH_BELOW) < 64.0 * TILED_MIN_MACS_DEFAULT <= criterion(SWITCH_ABOVE)
    # ... and with tiled_min_macs = 1 every other case is on the arrival-order side
    for c in ALL_CASES:
        assert criterion(c) >= 64.0, c.id


def test_batch_size_matches_the_source():
    """NW places the batch-boundary cases: it is the constant the kernels' DwfCfg<F64>::NW is defined by (WF_NW_F64,
    gft_wavefront_plan.hpp), read through the model library, which includes that header."""
    assert batch_rows() == NW


def test_model_on_a_hand_computed_case():
    """2 x 2, exact in binary64: exp(x)[1] = (1 x[1]) (*) res[0] / 1."""
    x = np.array([[0.0, 0.5], [0.25, 2.0]])
    row0 = np.array([1.0, 0.5])
    for descending in (False, True):
        got = exp_model(x, (2, 2), row0, descending)
        assert np.array_equal(got, [[1.0, 0.5], [0.25, 0.25 * 0.5 + 2.0 * 1.0]])


def test_families_are_what_the_planner_selects():
    """Every label of the case table against plan_wavefront itself, with and without `arrival_order`; every family is there."""
    for c in ALL_CASES:
        shape = case_data(c.id).want.shape
        if c.family in WAVEFRONT_FAMILIES:
            assert planned(shape, c.xn, True) == (c.family, 1), c.id
            assert planned(shape, c.xn, False) == (c.family, 0), c.id
        elif c.n[1] <= 4096:  # ("loop" with longer rows: exp_rec does not ask the planner, `wf_2d`)
            assert planned(shape, c.xn, True) == ("none", 0), c.id
    assert {c.family for c in ALL_CASES} >= set(WAVEFRONT_FAMILIES)
    assert planned((9, 4097), (9, 70)) == ("none", 0)
