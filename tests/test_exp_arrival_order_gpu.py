"""exp in arrival order on the device: the `rev` kernels against the DESCENDING ordered model, bit for bit.

Where Ops<E>::exp_rec (gft_ops_recur.inc) would take the right-looking tiled form, a rank-2 f64 exp runs the one-launch
wavefront with `rev` = 1 (k_div_wavefront<E, 1> packed and unpacked, k_div_wavefront_q<1, 8 | 16>, k_rows_wavefront:
gft_div2d.hip): every row's source rows in descending j0.  The library is built with -ffp-contract=off, so the model of
_exp_order_model.py — the same IEEE operations in that order, shown on the CPU to be the oracle's bits when it runs ascending
(test_exp_arrival_order_cpu.py) — must be reproduced exactly.  The other order of the same kernels (`exp_right` = 0, `rev` = 0)
must be the oracle's bits, and the host-driven right-looking loop (`div_wavefront` = 0) is held to the 1e-10 contract.

(test_div_row_wavefront_bit_exact covers the same kernels for div, log and exp with `rev` = 0 only.)"""
import numpy as np
import pytest

from _exp_order_model import CASES, SWITCH_ABOVE, SWITCH_BELOW, TILED_MIN_MACS_DEFAULT, WAVEFRONT_FAMILIES, case_data

pytestmark = pytest.mark.gpu

ONE_LAUNCH = 8  # the kernel + the fill of the result with the EMPTY pattern + the flags' memset + row 0 (test_div_row_wavefront_bit_exact's bound)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _where(a, b):
    return np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))[:5].tolist()


def _exp(GTP, d):
    """(array, launches of the exp alone), metadata checked against the oracle's."""
    import genfer_amd

    t = GTP.new(d.x, d.deg)
    before = genfer_amd.op_stats()["launches"]
    g = t.exp()
    launches = genfer_amd.op_stats()["launches"] - before
    assert g.degrees_p1() == d.degrees_p1
    got = g.array()
    assert got.shape == d.want.shape
    return got, launches


def _deviation(got, d):
    """max |got - oracle| / bound over the finite coefficients (a recorded figure: DESIGN, "exp in arrival order")."""
    with np.errstate(all="ignore"):
        r = np.abs(got - d.want) / d.bound
    r = r[np.isfinite(r)]
    return float(r.max()) if r.size else 0.0


def _within_contract(got, d):
    err = np.abs(got - d.want)
    assert np.all((err <= 1e-10 * d.bound) | (got == d.want)), (err / d.bound).max()


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_exp_arrival_order_is_the_descending_model(cid, GTP):
    import genfer_amd

    L = genfer_amd.lib()
    d = case_data(cid)
    wavefront = d.case.family in WAVEFRONT_FAMILIES
    finite = d.case.special in (None, "wide")
    assert L.gft_set_option(b"tiled_min_macs", 1.0) == 0  # the criterion holds for every case (test_switch_point_brackets_the_default_threshold)
    try:
        # ---- defaults otherwise: `rev` = 1 wherever the planner takes the shape
        got, launches = _exp(GTP, d)
        print(f"\n{cid}: family {d.case.family}, launches {launches}, max |got - oracle| / bound = {_deviation(got, d):.3e}")
        if wavefront:
            assert _same_bits(got, d.desc), ("not the descending order", _where(got, d.desc))
            assert launches <= ONE_LAUNCH, "exp did not take the one-launch wavefront"
        elif d.case.family == "line":  # a 1-d exp: the reference's order whatever the options say
            assert _same_bits(got, d.want), _where(got, d.want)
        else:  # "loop": the host-driven right-looking loop with tiled products
            _within_contract(got, d)
        # ---- `exp_right` = 0: the same kernels with `rev` = 0, the reference's order — the switch is what selects the order
        if wavefront or d.case.family == "line":
            assert L.gft_set_option(b"exp_right", 0.0) == 0
            try:
                got0, launches0 = _exp(GTP, d)
                assert _same_bits(got0, d.want), ("exp_right = 0 is not the oracle", _where(got0, d.want))
                if wavefront:
                    assert launches0 <= ONE_LAUNCH
            finally:
                L.gft_set_option(b"exp_right", 1.0)
        # ---- `div_wavefront` = 0: the right-looking loop adds with the tiled or reference-order product — the contract only
        # (not for the inf / nan cases, on purpose: their bound is not finite, so `err <= 1e-10 bound` would hold or fail for
        # reasons that say nothing about the loop; non-finite data is pinned above, bit for bit, in both orders)
        if finite:
            assert L.gft_set_option(b"div_wavefront", 0.0) == 0
            try:
                gotl, _ = _exp(GTP, d)
                _within_contract(gotl, d)
            finally:
                L.gft_set_option(b"div_wavefront", 1.0)
    finally:
        L.gft_set_option(b"tiled_min_macs", TILED_MIN_MACS_DEFAULT)


def test_exp_switches_to_arrival_order_at_the_default_threshold(GTP):
    """No option touched (`exp_right` on, `tiled_min_macs` = 2e5, `conv_mode` 0): 84 x 84 is the last full square below
    64 `tiled_min_macs` — the oracle's bits —, 85 x 85 the first one above — the descending model's.  A drift of the dispatch
    criterion fails here instead of silently changing which contract a shape gets."""
    below, above = case_data(SWITCH_BELOW.id), case_data(SWITCH_ABOVE.id)
    got, launches = _exp(GTP, below)
    assert _same_bits(got, below.want), ("84 x 84 left the reference's order", _where(got, below.want))
    assert launches <= ONE_LAUNCH
    got, launches = _exp(GTP, above)
    print(f"\n{SWITCH_ABOVE.id}: launches {launches}, max |got - oracle| / bound = {_deviation(got, above):.3e}")
    assert _same_bits(got, above.desc), ("85 x 85 is not in arrival order", _where(got, above.desc))
    assert launches <= ONE_LAUNCH
