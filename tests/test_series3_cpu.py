"""Batched trivariate series (genfer_amd.series3, gft_series3_*) without a GPU: the plain-Python model of the two shape rules and
the four recursions against the CPU oracle, the one-ulp sentinel of rule 1, the exported and declared surface and the refusals
the Python side makes before it touches a device."""
import itertools
import os
import re

import numpy as np
import pytest

import _series3_model as model
import make_series_refusals as table
from _series3_oracle import OPS, bits_equal, dense, model_batch, oracle_is_normative, signed, want
from conftest import ROOT

RESULTS = [(3, 3, 3), (4, 2, 3), (2, 4, 2), (3, 1, 3), (1, 2, 3), (2, 2, 1)]
FULL = [(2, 2, 2), (3, 4, 5), (5, 3, 2), (4, 4, 4), (2, 5, 7), (6, 2, 3), (3, 4, 1), (1, 3, 4), (4, 1, 1), (1, 1, 5)]
SYMBOLS = ("gft_series3_mul", "gft_series3_div", "gft_series3_exp", "gft_series3_log")


def stored_lengths(n):
    """every combination of {1, n_a - 1, n_a} per axis"""
    return list(itertools.product(*[sorted({1, max(1, na - 1), na}) for na in n]))


@pytest.mark.parametrize("op", OPS)
def test_model_against_the_oracle(op, OTP, oracle_lib):
    """0 differing bits, signs of zeros included, wherever the oracle is normative: every stored length of every operand axis under
    the six result shapes, dense and mixed signs; and full-shape operands at the ten further shapes"""
    checked = 0
    for n in RESULTS:
        shapes = stored_lengths(n)
        for xs in shapes:
            for ys in shapes if op in ("mul", "div") else [n]:
                for make in (dense, signed):
                    x, y = make((1,) + xs, 7 * n[0] + n[1]), make((1,) + ys, 11 * n[0] + n[2])
                    if not oracle_is_normative(op, x, y):
                        continue
                    ok = bits_equal(model_batch(op, x, y, n), want(oracle_lib, OTP, op, x, y, n))
                    assert ok.all(), (op, n, xs, ys, make.__name__)
                    checked += 1
    assert checked == {"mul": 2660, "div": 2508, "exp": 152, "log": 152}[op]  # 5 472 in all; div: less the one-coefficient divisors
    for n in FULL:
        x, y = dense((1,) + n, 3), dense((1,) + n, 4)
        assert bits_equal(model_batch(op, x, y, n), want(oracle_lib, OTP, op, x, y, n)).all(), (op, n)


def test_computing_on_n_instead_of_S_is_a_different_association(OTP, oracle_lib):
    """rule 1's sentinel: exp of a dense x stored as (4, 2, 1) at the result (5, 3, 2).  S = (5, 3, 1) -- the rank-2 loops -- carries
    the oracle's bits; the rank-3 loops run on n differ from it (by one ulp, in a few coefficients of column 0)"""
    x, n = dense((1, 4, 2, 1), 5), (5, 3, 2)
    assert model.result_shape("exp", n, x.shape[1:]) == (5, 3, 1)
    exp = want(oracle_lib, OTP, "exp", x, None, n)[0]
    assert bits_equal(model.exp(x[0], n), exp).all()
    off = ~bits_equal(model.exp(x[0], n, on=n), exp)
    assert off.any() and not off[:, :, 1].any()
    got = model.exp(x[0], n, on=n)
    assert np.all(np.abs(got[off] - exp[off]) <= 2 * np.spacing(np.abs(exp[off])))


def test_result_shape_rules():
    assert model.result_shape("mul", (4, 3, 2), (2, 2, 1), (2, 1, 1)) == (3, 2, 1)
    assert model.result_shape("div", (4, 3, 2), (4, 2, 2), (4, 1, 2)) == (4, 2, 2)
    assert model.result_shape("exp", (5, 3, 2), (4, 2, 1)) == (5, 3, 1) == model.result_shape("log", (5, 3, 2), (4, 2, 1))


def test_symbols_are_declared_and_exported():
    import genfer_amd

    if not os.path.exists(genfer_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    L = genfer_amd.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert hasattr(L, s), s
        assert f"pub fn {s}(" in doc, s


def test_module_is_re_exported():
    import genfer_amd
    from genfer_amd import series3

    assert genfer_amd.series3 is series3
    for f in OPS:
        assert callable(getattr(series3, f))
    assert series3.MAX_ELEMS == 4096


def test_python_side_refusals_need_no_device():
    """storage-less tensors that report a GPU placement reach every check in front of the library"""
    torch = pytest.importorskip("torch")
    from genfer_amd import series3
    from genfer_amd.taylor import TaylorError

    def T(*shape, **kw):
        return table._tensor(torch, dict({"t": list(shape)}, **kw))

    x = T(3, 2, 4, 8)
    binary, unary = (series3.mul, series3.div), (series3.exp, series3.log)
    for f in binary + unary:
        call = (lambda *a, **k: f(a[0], a[0], *a[1:], **k)) if f in binary else f  # noqa: E731
        with pytest.raises(TaylorError, match=r"n0 \* n1 \* n2 = 17 \* 241 \* 1 = 4097 exceeds the limit of 4096"):
            call(T(3, 1, 1, 1), n=(17, 241, 1))
        for n in [(1, 4, 8), (2, 3, 8), (2, 4, 7)]:  # an operand longer than n, on each axis
            with pytest.raises(TaylorError, match="nx > n"):
                call(x, n=n)
        for empty in [T(3, 0, 4, 8), T(3, 2, 0, 8), T(3, 2, 4, 0)]:
            with pytest.raises(TaylorError, match="is empty"):
                call(empty)
        with pytest.raises(TaylorError, match="n == 0"):
            call(x, n=(2, 0, 8))
        with pytest.raises(TaylorError, match="float32"):
            call(T(3, 2, 4, 8, dtype="float32"))
        with pytest.raises(TaylorError, match="at least 3"):
            call(T(4, 8))
        with pytest.raises(TaylorError, match="unit stride"):
            call(T(3, 2, 4, 8, step=2))
        with pytest.raises(TaylorError, match=r"out has \(2, 4, 9\)"):
            call(x, out=T(3, 2, 4, 9))
        with pytest.raises(TaylorError, match="batch shape"):
            call(x, out=T(1, 2, 4, 8))
        with pytest.raises(TaylorError, match="no autograd"):
            call(T(3, 2, 4, 8, grad=True))
        with pytest.raises(TaylorError, match="on cpu"):  # everything else in order: the placement is judged last
            call(T(3, 2, 4, 8, on="cpu"))
        with pytest.raises(TypeError, match="torch.Tensor"):
            call([[[1.0, 2.0]]])
        with pytest.raises(TypeError, match="triple"):
            call(x, n=(4, 8))
    for f in unary:  # a seed of the wrong shape: one value per item
        with pytest.raises(RuntimeError, match="broadcast"):  # (torch's own message for shapes that do not broadcast)
            f(x, seed=T(5))
        with pytest.raises(RuntimeError, match="broadcast"):
            f(x, seed=T(5), out=T(3, 2, 4, 8))
        with pytest.raises(TaylorError, match="batch shape"):  # a seed that broadcasts beyond the batch of out
            f(x, seed=T(2, 3), out=T(3, 2, 4, 8))
        with pytest.raises(TaylorError, match="float32"):
            f(x, seed=T(3, dtype="float32"))
    with pytest.raises(TaylorError, match="nx > n"):
        series3.mul(T(3, 1, 4, 8), x, n=(1, 4, 8))  # y is the long one
