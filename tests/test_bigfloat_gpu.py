"""EBig (genfer_amd/csrc/gft_elem.hpp) in a gfx950 kernel: the same seeded operand pairs as the CPU sweep of
tests/test_bigfloat_cpu.py, through tests/bigfloat_elem_check.hip --device, bit for bit against the element's host
pass and the test oracle's BigFloat (a NaN factor only has to be a NaN: its sign is the hardware's)."""
import numpy as np
import pytest

from test_bigfloat_cpu import ELEM_OPS, elem_check, gfh, orcb, orcb_path, random_pairs, run_elem, same, scalar_op  # noqa: F401


@pytest.mark.gpu
def test_ebig_device_matches_host_and_oracle(elem_check, orcb, tmp_path):  # noqa: F811
    pairs = random_pairs(100_000, 11)
    dev = run_elem(elem_check, pairs, tmp_path, device=True)
    host = run_elem(elem_check, pairs, tmp_path)
    bad = [(i, k) for i in range(len(pairs)) for k in range(len(ELEM_OPS)) if not same(dev[i][k], host[i][k])]
    assert not bad, f"{len(bad)} device/host mismatches, first: {[(ELEM_OPS[k], pairs[i], dev[i][k], host[i][k]) for i, k in bad[:3]]}"
    # and the oracle on a slice (the host pass is pinned against it on the full CPU sweep)
    for i in range(0, len(pairs), 10):
        a, b = pairs[i, :2], pairs[i, 2:]
        for op in ("add", "sub", "mul", "div", "neg", "normalize"):
            assert same(dev[i][ELEM_OPS.index(op)], scalar_op(orcb, "orcb_scalar_op", op, a, b)), (op, a, b)


@pytest.mark.gpu
def test_ebig_device_named_vectors(elem_check, tmp_path):  # noqa: F811
    from test_bigfloat_cpu import DOC_VECTORS, QUIRKS

    pairs = [list(a) + list(b if b is not None else (0.0, 0.0)) for _, a, b, _ in DOC_VECTORS + QUIRKS]
    dev = run_elem(elem_check, pairs, tmp_path, device=True)
    for (op, a, b, want), r in zip(DOC_VECTORS + QUIRKS, dev):
        assert same(r[ELEM_OPS.index(op)], np.array(want, dtype=np.float64)), (op, a, b, r[ELEM_OPS.index(op)])
