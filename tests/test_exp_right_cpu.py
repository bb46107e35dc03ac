"""CPU twin of test_exp_right_gpu.py: the exact rational exponential (_exp_exact.py) against closed forms, and the ORACLE
against it on every case of the GPU file under the project's contract  |got - exact| <= 1e-10 M  (M: the exact exponential
of |a|), so that a failure of the GPU file is the kernel's and not the reference's.

Measured worst ratio |oracle - exact| / M over all cases, both sign patterns: 9.4e-16 (see test_oracle_meets_the_contract)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from _exp_exact import CASES, case_reference, exp_series, result_shape, to_fractions, worst_ratio

CONTRACT = Fraction(1, 10 ** 10)


def test_exact_exp_closed_forms():
    """exp(x) = sum x^k / k!; exp(x + y) = exp(x) exp(y): E[i, j] = 1 / (i! j!); exp(x y z): 1 / k! on the diagonal."""
    f = to_fractions(np.array([0.0, 1.0]))
    assert list(exp_series(f, (7,))) == [Fraction(1, math.factorial(k)) for k in range(7)]
    f = to_fractions(np.array([[0.0, 1.0], [1.0, 0.0]]))
    E = exp_series(f, (5, 6))
    assert all(E[i, j] == Fraction(1, math.factorial(i) * math.factorial(j)) for i in range(5) for j in range(6))
    f = to_fractions(np.zeros((2, 2, 2)))
    f[1, 1, 1] = Fraction(1, 2)
    E = exp_series(f, (4, 3, 5))
    for i in np.ndindex(E.shape):
        assert E[i] == (Fraction(1, 2 ** i[0] * math.factorial(i[0])) if i[0] == i[1] == i[2] else 0)


def test_exact_exp_compact_operand_and_unit_axes():
    """A compact operand equals the same operand padded with zeros; a unit axis stays out of the recurrence."""
    rng = np.random.default_rng(3)
    a = rng.integers(-4, 5, size=(2, 3, 2)).astype(np.float64) / 8.0
    a[0, 0, 0] = 0.0
    padded = np.zeros((4, 3, 5))
    padded[:2, :3, :2] = a
    assert np.array_equal(exp_series(to_fractions(a), (4, 3, 5)), exp_series(to_fractions(padded), (4, 3, 5)))
    b = a[:, :1, :]
    assert np.array_equal(exp_series(to_fractions(b), (4, 1, 5))[:, 0, :], exp_series(to_fractions(b[:, 0, :]), (4, 5)))


@pytest.mark.parametrize("positive", [False, True], ids=["mixed", "positive"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_meets_the_contract(name, positive, OTP):
    """The oracle alone, every case: the seed within 4 ulp of libm's exp(c0), every coefficient within 1e-10 M of
    seed * E (positive arguments: M = E, i.e. 1e-10 relative per coefficient).  Worst ratio measured: 9.4e-16 (last_over_128, positive)."""
    deg, xs, _ = CASES[name]
    a, c0, E, M = case_reference(name, positive)
    got = np.asarray(OTP.new(a, list(deg)).exp().array())
    assert got.shape == result_shape(deg, xs)
    seed = got[(0,) * got.ndim]
    assert abs(seed - math.exp(c0)) <= 4 * math.ulp(math.exp(c0))
    ratio = worst_ratio(got, E, M, seed)
    print(f"oracle {name} {'positive' if positive else 'mixed'}: worst ratio {float(ratio):.3e}")
    assert ratio <= CONTRACT, float(ratio)
