"""pow through the one driver of ranks 1, 2 and 3 (gft_series.hip series_pow over gft_series_args.hpp series_pow_steps) on the MI355X.

One shape per rank at which truncation starts in the middle of the chain (rank 3 with a unit axis in x), a batch of (2, 3), f64 and
intervals, e in {0, 1, 2, 3, 6, 7}, and three placements: contiguous; x broadcast along the first batch axis (stride 0); the result
in place on x (x of shape n).  Every coefficient carries the bits of the chain of oracle products that defines pow (want_pow of each
rank's case module), never the library's own pow.  gft_series_last_form() reports what it reported before the ranks shared a driver:
at rank 1 None for e = 0, else the form of the last product ("B": six series are fewer than form A takes by itself); "B" above."""
import numpy as np
import pytest

import _series2_compose_cases as cc2
import _series3_compose_cases as cc3
import test_interval_series2_cpu as iv2
import test_interval_series3_cpu as iv3
import test_interval_series_cpu as iv1
import test_series_compose_cpu as cc1
from _series2_oracle import assert_bits
from test_interval_series2_cpu import shim2  # noqa: F401
from test_interval_series3_cpu import shim3  # noqa: F401
from test_interval_series_cpu import shim  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
BATCH = (2, 3)
EXPONENTS = (0, 1, 2, 3, 6, 7)
SHAPES = {1: ((3,), (8,)), 2: ((2, 3), (3, 8)), 3: ((2, 1, 3), (3, 2, 5))}  # rank: (the stored shape of x, the orders n)
PLACEMENTS = ("contiguous", "broadcast", "in place")


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def module(rank, w):
    import importlib

    return importlib.import_module("genfer_amd." + ("interval_series" if w == 2 else "series") + ("" if rank == 1 else str(rank)))


def operand(rank, w, B, shape, seed):
    """B items: f64 [B, shape...], intervals [2, B, shape...]"""
    if w == 1:
        return (cc1.dense, cc2.dense, cc3.dense)[rank - 1]((B,) + shape, seed)
    if rank == 1:
        return iv1.data("mixed", B, shape[0], seed)
    return iv2.data2("mixed", B, shape, seed) if rank == 2 else iv3.data3("signed", B, shape, seed)


def want(request, rank, w, X, e, n):
    """want_pow of the rank's case module on the B items of X"""
    if w == 1:
        lib = request.getfixturevalue("oracle_lib")
        return cc1.want_pow(lib, X, e, n[0]) if rank == 1 else (cc2 if rank == 2 else cc3).want_pow(lib, X, e, n)
    if rank == 1:
        return iv1.want_pow(request.getfixturevalue("shim"), X, e, n[0])
    return (iv2 if rank == 2 else iv3).want_pow(request.getfixturevalue("shim" + str(rank)), X, e, n)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("w", (1, 2), ids=("f64", "interval"))
@pytest.mark.parametrize("rank", (1, 2, 3))
def test_pow_bits_and_form(request, rank, w, placement):
    from genfer_amd import series

    xs, n = SHAPES[rank]
    mod = module(rank, w)
    lead = (2,) if w == 2 else ()  # the planes of an interval tensor
    B = BATCH[1] if placement == "broadcast" else BATCH[0] * BATCH[1]
    X = operand(rank, w, B, n if placement == "in place" else xs, 100 * rank + 10 * w + len(placement))
    norder = n[0] if rank == 1 else n
    for e in EXPONENTS:
        exp = want(request, rank, w, X, e, n)
        if placement == "broadcast":  # the three items serve both rows of the batch
            x = dev(X).reshape(lead + (1, BATCH[1]) + X.shape[len(lead) + 1:]).expand(lead + BATCH + X.shape[len(lead) + 1:])
            assert x.stride(len(lead)) == 0
            exp = np.concatenate([exp, exp], axis=len(lead))
            got = mod.pow(x, e, n=norder)
        elif placement == "in place":
            x = dev(X).reshape(lead + BATCH + n)
            got = mod.pow(x, e, out=x)
            assert got.data_ptr() == x.data_ptr()
        else:
            got = mod.pow(dev(X).reshape(lead + BATCH + xs), e, n=norder)
        form = series.last_form()
        assert form == (None if rank == 1 and e == 0 else "B"), (rank, w, placement, e, form)
        assert_bits(got.reshape(exp.shape), exp, f"pow rank {rank} w={w} {placement} e={e}")
