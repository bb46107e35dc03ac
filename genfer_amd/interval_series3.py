"""Batched trivariate series on interval device tensors: ``mul``, ``div``, ``exp``, ``log``, ``compose``, ``pow``
(``gfti_series3_*``), the ``Interval<F64>`` half of ``genfer_amd.series3``.

An interval tensor is float64 and stacked ``[2, B..., n0, n1, n2]`` = (lo, hi) along its first axis, as
``IntervalTaylorPoly.from_torch`` takes it.  The last three axes are the coefficient array of one ``TaylorPoly<Interval<F64>>`` in
three variables (axis -3: variable 0, the slabs, and axis -2: variable 1, the rows, both with any non-negative stride; axis -1:
variable 2, unit stride), the axes between are batch axes and broadcast by torch's rules.  The plane axis may have any non-negative
stride on an operand, 0 included: ``x.expand(2, ...)`` is a batch of point intervals, no copy.  The result's two planes are distinct
memory.  Seeds of ``exp`` / ``log`` are ``[2, B...]``.  ``n0 * n1 * n2 <= 2048``: an interval takes 16 bytes of LDS, so the footprints
float64 items reach at 4096 are reached there.  Per item the results are the recursions of ``genfer_amd.series3`` -- the stored
result shape ``S``, its squeeze and the ``[+0.0, +0.0]`` outside it included -- with every step one operation of the reference's
interval arithmetic (round to nearest, one ulp outwards, its short-circuits included), every bound with the oracle's bits.  One
launch per call (``pow``: a sequence inside one call), one workgroup per item; the call is ordered on torch's current stream and does
not wait.

    >>> from genfer_amd import interval_series3 as ivs3
    >>> z = ivs3.mul(x, y)                              # x, y: [2, B, n0, n1, n2] float64 on the GPU
    >>> q = ivs3.div(p.expand(2, B, n0, n1, n2), y)     # p: [B, n0, n1, n2] point values
    >>> e = ivs3.exp(x, seed=s)                         # s: [2, B], the interval exp of coefficient [0, 0, 0]
    >>> h = ivs3.compose(f, g, var=2)
    >>> p = ivs3.pow(x, 5)

No autograd: an operand that requires grad is refused while grad mode is on, as in ``series3``.
"""
from __future__ import annotations

from ._series_call import Call
from ._series_call import run as _run
from .series import _exponent
from .series3 import _var

MAX_ELEMS = 2048  # gft_series_args.hpp SERIES3_MAX_ELEMS_IV: n0 * n1 * n2 of the result

_CALL = Call("interval_series3", 3, 1, MAX_ELEMS, raw=True)


def mul(x, y, n=None, out=None):
    """``z[b] = x[b] * y[b]`` truncated at orders ``n = (n0, n1, n2)`` (default: the larger stored length on each axis): the general
    product over intervals."""
    return _run(_CALL, "mul", x, y, n, out)


def div(x, y, n=None, out=None):
    """``r[b] = x[b] / y[b]`` to orders ``n``: the general division recurrence over the slabs, over intervals."""
    return _run(_CALL, "div", x, y, n, out)


def exp(x, n=None, seed=None, out=None):
    """``exp(x[b])`` to orders ``n``.  ``seed``: the interval ``exp`` of coefficient ``[0, 0, 0]`` per item, ``[2, B...]``; with the
    host libm's values widened as the reference widens them the result carries its bits.  ``None``: formed on the device."""
    return _run(_CALL, "exp", x, seed, n, out)


def log(x, n=None, seed=None, out=None):
    """``log(x[b])`` to orders ``n``.  ``seed``: the interval ``ln`` of coefficient ``[0, 0, 0]`` per item, ``[2, B...]``; ``None``:
    formed on the device (only coefficient ``[0, 0, 0]`` depends on it)."""
    return _run(_CALL, "log", x, seed, n, out)


def compose(f, g, var=0, n=None, out=None):
    """``f[b]`` with ``g[b]`` substituted for variable ``var`` (0: axis -3, 1: axis -2, 2: axis -1) of ``f``, truncated at
    ``n = (n0, n1, n2)``: ``series3.compose``'s Horner loop with the general interval product at every step, the whole loop in one
    launch.  ``out`` may be ``f`` or ``g`` itself."""
    return _run(_CALL, "compose", f, g, n, out, var=_var("interval_series3.compose", var))


def pow(x, e, n=None, out=None):  # noqa: A001 (the reference's name)
    """``x[b] ** e`` truncated at ``n = (n0, n1, n2)`` (default: the stored shape) for an integer ``0 <= e < 2**32``: the reference's
    square-and-multiply over ``mul`` at compact shapes.  ``e = 0`` gives the unit item: ``[1, 1]`` at ``[0, 0, 0]``, ``[0, 0]``
    elsewhere.  ``out`` may be ``x`` itself."""
    e = _exponent("interval_series3.pow", e, div="interval_series3.div")
    return _run(_CALL, "pow", x, None, n, out, scalar=e)
