"""Batched univariate series on interval device tensors: ``mul``, ``div``, ``exp``, ``log``, ``compose``, ``pow`` and the
observation ops ``derivative``, ``taylor_expansion_of_coeff``, ``shift_down``, ``evaluate_all_one`` (``gfti_series_*``), the ``Interval<F64>`` half of ``genfer_amd.series``.

An interval tensor is float64 and stacked ``[2, B..., n]`` = (lo, hi) along its first axis, as ``IntervalTaylorPoly.from_torch``
takes it.  The last axis is the series (unit stride), the axes between are batch axes and broadcast by torch's rules.  The
plane axis may have any non-negative stride on an operand, 0 included: ``x.expand(2, ...)`` is a batch of point intervals, no
copy.  The result's two planes are distinct memory.  Seeds of ``exp`` / ``log`` are ``[2, B...]``.  Item ``b`` is the
``TaylorPoly<Interval<F64>>`` of one variable with coefficients ``[x[0, b, k], x[1, b, k]]`` and truncation order ``n <= 2048``
(two planes reach at 2048 the footprints float64 rows reach at 4096).  Per item the results are the reference's *general*
algorithms over its interval arithmetic (round to nearest, one ulp outwards), every bound with the oracle's bits, and none of
the operators' shortcuts.  The call is ordered on torch's current stream and does not wait.

    >>> from genfer_amd import interval_series as ivs
    >>> z = ivs.mul(x, y)                          # x, y: [2, B, n] float64 on the GPU
    >>> q = ivs.div(p.expand(2, B, n), y)          # p: [B, n] point values
    >>> e = ivs.exp(x, seed=s)                     # s: [2, B], the interval exp of coefficient 0
    >>> h = ivs.compose(f, g)
    >>> p = ivs.pow(x, 5)
"""
from __future__ import annotations

from ._series_call import Call
from .series import FORMS, _exponent, _run, last_form, set_form  # noqa: F401  (one library, one form option, one last form)

MAX_N = 2048  # gft_series.hpp SERIES_MAX_N_IV


# The arithmetic ops do not refuse an operand that requires grad (they run on its values); the observation ops, like every op of
# interval_series2, do.  Kept as it is.
_CALL = Call("interval_series", 1, 1, MAX_N, raw=False)
_OBSERVE = _CALL._replace(raw=True)


def mul(x, y, n=None, out=None):
    """``z[b] = x[b] * y[b]`` truncated at order ``n`` (default ``max(nx, ny)``): the general product ``mul_1d`` over intervals."""
    return _run(_CALL, "mul", x, y, n, out)


def div(x, y, n=None, out=None):
    """``r[b] = x[b] / y[b]`` to order ``n`` (default ``max(nx, ny)``): the general division recurrence over intervals."""
    return _run(_CALL, "div", x, y, n, out)


def exp(x, n=None, seed=None, out=None):
    """``exp(x[b])`` to order ``n`` (default ``nx``).  ``seed``: the interval ``exp`` of coefficient 0 per item, ``[2, B...]``; with
    the host libm's values widened as the reference widens them the result carries its bits.  ``None``: formed on the device."""
    return _run(_CALL, "exp", x, seed, n, out)


def log(x, n=None, seed=None, out=None):
    """``log(x[b])`` to order ``n`` (default ``nx``).  ``seed``: the interval ``ln`` of coefficient 0 per item, ``[2, B...]``;
    ``None``: formed on the device (only coefficient 0 depends on it)."""
    return _run(_CALL, "log", x, seed, n, out)


def compose(f, g, n=None, out=None):
    """``f[b](g[b])`` truncated at order ``n`` (default ``max(nf, ng)``): Horner over the coefficients of ``f`` with the general
    interval product at every step, as ``series.compose``.  About ``nf * n**2 / 2`` interval multiply-adds per item, on one
    workgroup at most."""
    return _run(_CALL, "compose", f, g, n, out)


def pow(x, e, n=None, out=None):  # noqa: A001 (the reference's name)
    """``x[b] ** e`` truncated at order ``n`` (default ``nx``) for an integer ``0 <= e < 2**32``: the reference's
    square-and-multiply over ``mul`` at compact lengths.  ``e = 0`` gives ``[[1, 1], [0, 0], ...]``."""
    return _run(_CALL, "pow", x, None, n, out, scalar=_exponent("interval_series.pow", e, div="interval_series.div"))


# ---- the observation ops: series.derivative / taylor_expansion_of_coeff / shift_down / evaluate_all_one over intervals --------
# (no autograd here: an operand that requires grad is refused while grad mode is on)


def derivative(x, k, out=None):
    """``out[:, b, j] = x[:, b, k + j] * ff_j`` with the reference's interval factors ``ff_j`` (``series.derivative``'s recurrence in
    interval arithmetic); ``[2, B..., nx - k]``."""
    return _run(_OBSERVE, "derivative", x, out=out, scalar=k)


def taylor_expansion_of_coeff(x, k, out=None):
    """Coefficient ``k`` untouched, coefficient ``k + j`` times the interval factor ``f_j`` for ``j >= 1``."""
    return _run(_OBSERVE, "taylor_expansion_of_coeff", x, out=out, scalar=k)


def shift_down(x, k, out=None):
    """``out[:, b, 0] = x[:, b, k] + S`` with ``S`` the ascending interval sum of coefficients ``0 .. k-1`` from ``[0, 0]`` (all of them
    when ``nx == k + 1``), the others copies."""
    return _run(_OBSERVE, "shift_down", x, out=out, scalar=k)


def evaluate_all_one(x, out=None):
    """The ascending interval sum of every item's coefficients from ``[0, 0]``; ``[2, B...]``."""
    return _run(_OBSERVE, "evaluate_all_one", x, out=out)


def observe_chain(a, x, cs, degree_p1=None, out=None):
    """``series.observe_chain`` over intervals: ``a`` is ``[2, B..., L]``, ``x`` ``[2, B...]`` or ``None`` (continuous rate), ``cs``
    ``[2, B..., nsteps]``; every product and sum is the reference's interval operation.  A scalar counts as 0 or 1 when both of its
    bounds are."""
    from ._series_call import run_chain

    return run_chain(_OBSERVE, a, None, x, cs, degree_p1, out)


def lah_row(p, order, out=None):
    """``series.lah_row`` over intervals: ``p`` is ``[2, B...]``, the result ``[2, B..., order + 1]``."""
    from ._series_call import run_lah_row

    return run_lah_row(_OBSERVE, p, order, out)


def observe_negbinomial(a, x, p, ls, degree_p1=None, out=None):
    """``series.observe_negbinomial`` over intervals: ``a`` is ``[2, B..., L]``, ``x`` and ``p`` ``[2, B...]``, ``ls``
    ``[2, B..., k + 1]``; ``3 * degree_p1 + k <= 4096``.  A scalar counts as 0 or 1 when both of its bounds are."""
    from ._series_call import run_negbinomial

    return run_negbinomial(_OBSERVE, a, None, x, p, ls, degree_p1, out)


def mul_linear(a, c, m, n=None, out=None):
    """``series.mul_linear`` over intervals: ``a`` is ``[2, B..., L]``, ``c`` and ``m`` ``[2, B...]``; every product and sum is the
    reference's interval operation, and ``c`` counts as 0 when both of its bounds are."""
    from ._series_call import run_linear

    return run_linear(_OBSERVE, "mul_linear", a, None, None, c, m, n, out)


def compose_linear(f, c, m, n=None, out=None):
    """``series.compose_linear`` over intervals: ``f`` is ``[2, B..., nf]``, ``c`` and ``m`` ``[2, B...]``."""
    from ._series_call import run_linear

    return run_linear(_OBSERVE, "compose_linear", f, None, None, c, m, n, out)
