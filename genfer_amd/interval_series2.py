"""Batched bivariate series on interval device tensors: ``mul``, ``div``, ``exp``, ``log``, ``compose``, ``pow`` and the
observation ops ``derivative``, ``taylor_expansion_of_coeff``, ``shift_down``, ``evaluate_all_one`` (``gfti_series2_*``), the ``Interval<F64>`` half of ``genfer_amd.series2``.

An interval tensor is float64 and stacked ``[2, B..., n0, n1]`` = (lo, hi) along its first axis, as ``IntervalTaylorPoly.from_torch``
takes it.  The last two axes are the coefficient array of one ``TaylorPoly<Interval<F64>>`` in two variables (axis -2: variable 0,
any non-negative stride; axis -1: variable 1, unit stride), the axes between are batch axes and broadcast by torch's rules.  The
plane axis may have any non-negative stride on an operand, 0 included: ``x.expand(2, ...)`` is a batch of point intervals, no
copy.  The result's two planes are distinct memory.  Seeds of ``exp`` / ``log`` are ``[2, B...]``.  ``n0 * n1 <= 2048``: an
interval takes 16 bytes of LDS, so the footprints float64 items reach at 4096 are reached there.  Per item the results are the
recursions of ``genfer_amd.series2`` with every step one operation of the reference's interval arithmetic (round to nearest, one
ulp outwards, its short-circuits included), every bound with the oracle's bits.  One launch per call (``pow``: a sequence inside
one call), one workgroup per item; the call is ordered on torch's current stream and does not wait.

    >>> from genfer_amd import interval_series2 as ivs2
    >>> z = ivs2.mul(x, y)                          # x, y: [2, B, n0, n1] float64 on the GPU
    >>> q = ivs2.div(p.expand(2, B, n0, n1), y)     # p: [B, n0, n1] point values
    >>> e = ivs2.exp(x, seed=s)                     # s: [2, B], the interval exp of coefficient [0, 0]
    >>> h = ivs2.compose(f, g, var=1)
    >>> p = ivs2.pow(x, 5)

No autograd: an operand that requires grad is refused while grad mode is on, as in ``series2``.
"""
from __future__ import annotations

from ._series_call import Call
from .series import _exponent
from .series2 import _run, _var

MAX_ELEMS = 2048  # gft_series.hpp SERIES2_MAX_ELEMS_IV: n0 * n1 of the result


_CALL = Call("interval_series2", 2, 1, MAX_ELEMS, raw=True)


def mul(x, y, n=None, out=None):
    """``z[b] = x[b] * y[b]`` truncated at orders ``n = (n0, n1)`` (default: the larger stored length on each axis): the general
    product over intervals."""
    return _run(_CALL, "mul", x, y, n, out)


def div(x, y, n=None, out=None):
    """``r[b] = x[b] / y[b]`` to orders ``n = (n0, n1)``: the general division recurrence over the rows, over intervals."""
    return _run(_CALL, "div", x, y, n, out)


def exp(x, n=None, seed=None, out=None):
    """``exp(x[b])`` to orders ``n``.  ``seed``: the interval ``exp`` of coefficient ``[0, 0]`` per item, ``[2, B...]``; with the host
    libm's values widened as the reference widens them the result carries its bits.  ``None``: formed on the device."""
    return _run(_CALL, "exp", x, seed, n, out)


def log(x, n=None, seed=None, out=None):
    """``log(x[b])`` to orders ``n``.  ``seed``: the interval ``ln`` of coefficient ``[0, 0]`` per item, ``[2, B...]``; ``None``:
    formed on the device (only coefficient ``[0, 0]`` depends on it)."""
    return _run(_CALL, "log", x, seed, n, out)


def compose(f, g, var=0, n=None, out=None):
    """``f[b]`` with ``g[b]`` substituted for variable ``var`` (0: axis -2, 1: axis -1) of ``f``, truncated at ``n = (n0, n1)``:
    ``series2.compose``'s Horner loop with the general interval product at every step, the whole loop in one launch."""
    return _run(_CALL, "compose", f, g, n, out, var=_var("interval_series2.compose", var))


def pow(x, e, n=None, out=None):  # noqa: A001 (the reference's name)
    """``x[b] ** e`` truncated at ``n = (n0, n1)`` (default: the stored shape) for an integer ``0 <= e < 2**32``: the reference's
    square-and-multiply over ``mul`` at compact shapes.  ``e = 0`` gives the unit item: ``[1, 1]`` at ``[0, 0]``, ``[0, 0]`` elsewhere."""
    e = _exponent("interval_series2.pow", e, div="interval_series2.div")
    return _run(_CALL, "pow", x, None, n, out, scalar=e)


# ---- the observation ops: series2's over intervals ----------------------------------------------------------------------------


def derivative(x, var, k, out=None):
    """``series2.derivative`` with the reference's interval factors; the axis of ``var`` is ``k`` shorter."""
    return _run(_CALL, "derivative", x, out=out, scalar=k, var=var)


def taylor_expansion_of_coeff(x, var, k, out=None):
    """``series2.taylor_expansion_of_coeff`` over intervals: slice ``k`` untouched, slice ``k + j`` times the interval ``f_j``."""
    return _run(_CALL, "taylor_expansion_of_coeff", x, out=out, scalar=k, var=var)


def shift_down(x, var, k, out=None):
    """``series2.shift_down`` over intervals: the same orders of summation, every step the reference's interval addition."""
    return _run(_CALL, "shift_down", x, out=out, scalar=k, var=var)


def evaluate_all_one(x, out=None):
    """The row-major interval sum of every item from ``[0, 0]``; ``[2, B...]``."""
    return _run(_CALL, "evaluate_all_one", x, out=out)


def observe_chain(a, var, x, cs, degree_p1=None, out=None):
    """``series2.observe_chain`` over intervals: ``a`` is ``[2, B..., n0, n1]``, ``x`` ``[2, B...]`` or ``None``, ``cs``
    ``[2, B..., nsteps]``."""
    from ._series_call import run_chain

    return run_chain(_CALL, a, var, x, cs, degree_p1, out)


def observe_negbinomial(a, var, x, p, ls, degree_p1=None, out=None):
    """``series2.observe_negbinomial`` over intervals: ``a`` is ``[2, B..., n0, n1]``, ``x`` and ``p`` ``[2, B...]``, ``ls``
    ``[2, B..., k + 1]`` (from ``interval_series.lah_row``)."""
    from ._series_call import run_negbinomial

    return run_negbinomial(_CALL, a, var, x, p, ls, degree_p1, out)


def mul_linear(a, var, c, m, n=None, out=None):
    """``series2.mul_linear`` over intervals: ``a`` is ``[2, B..., n0, n1]``, ``c`` and ``m`` ``[2, B...]``."""
    from ._series_call import run_linear

    return run_linear(_CALL, "mul_linear", a, var, None, c, m, n, out)


def compose_linear(f, var, c, m, wvar=None, n=None, out=None):
    """``series2.compose_linear`` over intervals: ``f`` is ``[2, B..., n0, n1]``, ``c`` and ``m`` ``[2, B...]``."""
    from ._series_call import run_linear

    return run_linear(_CALL, "compose_linear", f, var, wvar, c, m, n, out)
