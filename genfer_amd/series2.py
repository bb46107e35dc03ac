"""Batched bivariate series on float64 device tensors: ``mul``, ``div``, ``exp``, ``log``, ``compose``, ``pow`` and the transposed
product ``corr`` and the observation ops ``derivative``, ``taylor_expansion_of_coeff``, ``shift_down``, ``evaluate_all_one``
and the fused Poisson observation chain ``observe_chain`` (``gft_series2_*``).

The last two axes of every tensor are the coefficient array of one ``TaylorPoly<F64>`` in two variables: axis -2 is variable 0
(any non-negative stride), axis -1 is variable 1 (unit stride); the leading axes are batch axes and broadcast by torch's rules
(``expand``, no copy).  An operand of stored shape ``(nx0, nx1)`` smaller than the result's ``(n0, n1)`` is a compact operand.
Per item the results are the reference's *general* recursion over axis 0 in its operation order, with the univariate loops of
``genfer_amd.series`` on the rows -- none of the shortcuts the handle operators take, so a result never depends on what else is
in the batch (``include/gftaylor.h`` states the loops).  One launch per call, one workgroup per item; ``n0 * n1 <= 4096``.  The
call is ordered on torch's current stream and does not wait.  ``compose`` substitutes a series for one of the two variables
(``subst_var``'s Horner loop, the whole loop in one launch); ``pow`` is square-and-multiply over ``mul``'s launches inside one call.

    >>> from genfer_amd import series2
    >>> z = series2.mul(x, y)                      # x, y: [B, n0, n1] float64 on the GPU
    >>> q = series2.div(x, y[0])                   # every item by one series
    >>> e = series2.exp(x, seed=torch.exp(x[..., 0, 0]))
    >>> h = series2.compose(f, g, var=1)           # g for variable 1 of f
    >>> p = series2.pow(x, 5)

No autograd in this version of the module: it is the raw layer, and an operand that requires grad is refused while grad mode is on
(``detach()`` it, or use ``torch.no_grad()``).  The differentiable twins of the six operations are ``genfer_amd.series2_grad``; their
backward passes are sequences of this module's calls around ``corr`` (the adjoint of ``mul``) and ``_compose_adj`` (the transposed
Horner loop).  float64 only; the ``Interval<F64>`` twins on ``[2, B..., n0, n1]`` tensors are ``genfer_amd.interval_series2``.
"""
from __future__ import annotations

from ._series_call import Call, _lib  # noqa: F401  (one declared library for the four modules)
from ._series_call import run as _run
from .series import _exponent
from .taylor import TaylorError

MAX_ELEMS = 4096  # gft_series.hpp SERIES2_MAX_ELEMS: n0 * n1 of the result in this version

_CALL = Call("series2", 2, 0, MAX_ELEMS, raw=True)  # rank 2, one plane; the differentiable twin is series2_grad


def _orders(what, n, *shapes, max_elems=None):
    max_elems = MAX_ELEMS if max_elems is None else max_elems
    if n is None:
        n = (max(s[0] for s in shapes), max(s[1] for s in shapes))
    try:
        n0, n1 = (int(v) for v in n)
    except (TypeError, ValueError):
        raise TypeError(f"{what}: n must be a pair (n0, n1), got {n!r}") from None
    if n0 < 1 or n1 < 1:
        raise TaylorError(f"{what}: n = ({n0}, {n1}); the result needs at least one coefficient on each axis (n == 0 is refused)")
    if n0 * n1 > max_elems:
        raise TaylorError(f"{what}: n0 * n1 = {n0} * {n1} = {n0 * n1} exceeds the limit of {max_elems} coefficients per item of this version")
    for s in shapes:
        for a in (0, 1):
            if s[a] > (n0, n1)[a]:
                raise TaylorError(f"{what}: an operand has {s[a]} coefficients on axis {a - 2}, more than n{a} = {(n0, n1)[a]} (nx > n)")
    return n0, n1


def _orders_short(what, n, g, y, names):
    """corr / _compose_adj: the result (shape ``n``, default ``g``) is the short side of a transposed operation on both axes; the
    first operand (stored shape ``g``) carries the limit and bounds the second (``y``)"""
    if n is None:
        n = g
    try:
        n0, n1 = (int(v) for v in n)
    except (TypeError, ValueError):
        raise TypeError(f"{what}: {names[2]} must be a pair, got {n!r}") from None
    if n0 < 1 or n1 < 1:
        raise TaylorError(f"{what}: {names[2]} = ({n0}, {n1}); the result needs at least one coefficient on each axis")
    if g[0] * g[1] > MAX_ELEMS:
        raise TaylorError(f"{what}: {names[0]} has {g[0]} * {g[1]} = {g[0] * g[1]} coefficients, which exceeds the limit of {MAX_ELEMS} per item "
                          "of this version")
    for a in (0, 1):
        if (n0, n1)[a] > g[a]:
            raise TaylorError(f"{what}: {names[2]} = ({n0}, {n1}) exceeds the {tuple(g)} coefficients of {names[0]} on axis {a - 2} (the result of "
                              "a transposed operation is its short side)")
    for a in (0, 1):
        if y[a] > g[a]:
            raise TaylorError(f"{what}: {names[1]} has {y[a]} coefficients on axis {a - 2}, more than the {g[a]} of {names[0]}")
    return n0, n1


def mul(x, y, n=None, out=None):
    """``z[b] = x[b] * y[b]`` truncated at orders ``n = (n0, n1)`` (default: the larger stored length on each axis)."""
    return _run(_CALL, "mul", x, y, n, out)


def div(x, y, n=None, out=None):
    """``r[b] = x[b] / y[b]`` to orders ``n = (n0, n1)``: the general division recurrence over the rows."""
    return _run(_CALL, "div", x, y, n, out)


def exp(x, n=None, seed=None, out=None):
    """``exp(x[b])`` to orders ``n``.  ``seed``: ``exp(x[b, 0, 0])`` per item (a tensor of the batch shape); with the host libm's
    values the result carries the reference's bits.  ``None``: formed on the device (a few ulps from libm)."""
    return _run(_CALL, "exp", x, seed, n, out)


def log(x, n=None, seed=None, out=None):
    """``log(x[b])`` to orders ``n``.  ``seed``: ``ln(x[b, 0, 0])`` per item; ``None``: formed on the device (only coefficient
    ``[0, 0]`` depends on it)."""
    return _run(_CALL, "log", x, seed, n, out)


def compose(f, g, var=0, n=None, out=None):
    """``f[b]`` with ``g[b]`` substituted for variable ``var`` (0: axis -2, 1: axis -1) of ``f``, truncated at ``n = (n0, n1)``
    (default: the larger stored length on each axis).  ``subst_var``'s general Horner path without its shortcuts: over the slices
    of ``f`` along the substituted axis, ``res = res * g + slice`` with the general product at the compact shape of every step,
    from ``res = 0.0 + the last slice``; the result stays in LDS across the steps of the one launch.  Cost: about
    ``nslices * (n0*n1)**2 / 4`` multiply-adds per item, all on one workgroup; no cap is imposed."""
    return _run(_CALL, "compose", f, g, n, out, var=_var("series2.compose", var))


def _var(what, var, role="the variable of f that g replaces is 0 or 1"):
    """the one check of a variable's index, for every module (the observation ops state their own role)"""
    if isinstance(var, bool) or not isinstance(var, int) or var not in (0, 1):
        raise TaylorError(f"{what}: var = {var!r}; {role}")
    return var


def corr(g, y, m=None, out=None):
    """The transposed product, the adjoint of ``mul``: ``<mul(x, y, g.shape), g> = <x, corr(g, y)>``.  ``g`` has stored shape
    ``(g0, g1)`` with ``g0 * g1 <= 4096``, ``y`` has ``(ny0, ny1) <= (g0, g1)`` per axis, the result ``m = (m0, m1) <= (g0, g1)``
    per axis (default: ``g``'s stored shape)::

        c[b, i0, i1] = 0.0 + sum_k0 (0.0 + sum_k1 g[b, k0, k1] * y[b, k0 - i0, k1 - i1])

    with ``k0`` descending from ``min(g0 - 1, i0 + ny0 - 1)`` to ``i0`` and ``k1`` from ``min(g1 - 1, i1 + ny1 - 1)`` to ``i1``,
    multiply and add rounded separately, only stored coefficients entering a sum: bit for bit ``mul(flip(g), y, n=g.shape)`` at
    index ``[g0 - 1 - i0, g1 - 1 - i1]``, ``flip`` reversing both series axes.  ``out`` may be ``g`` itself, never ``y``."""
    return _run(_CALL, "corr", g, y, m, out)


def _compose_adj(gh, g, var, nf, out=None):
    """The transposed Horner loop: the gradient of ``compose(f, g, var, n)`` with respect to ``f`` (stored shape ``nf``) from the
    gradient ``gh`` of the composition (shape ``n``).  With ``S`` slices of ``f`` of ``len`` coefficients along axis ``var`` and
    ``L_i = min(base + (S - 1 - i) * (ng - 1), n)`` per axis, ``base = (1, len)`` / ``(len, 1)``: ``a = gh[:L_0]``; slice ``i`` of the
    result is the first ``len`` entries of row 0 (var 0) / column 0 (var 1) of ``a``; then ``a = corr(a, g, L_{i+1})`` -- in one launch."""
    return _run(_CALL, "compose_adj", gh, g, nf, out, var=_var("series2._compose_adj", var))


def pow(x, e, n=None, out=None):  # noqa: A001 (the reference's name)
    """``x[b] ** e`` truncated at ``n = (n0, n1)`` (default: the stored shape) for an integer ``0 <= e < 2**32``: the reference's
    square-and-multiply over ``mul`` at compact shapes.  ``e = 0`` gives the unit item ``[[1, 0, ...], [0, ...], ...]``."""
    e = _exponent("series2.pow", e, div="series2.div")
    return _run(_CALL, "pow", x, None, n, out, scalar=e)


# ---- the observation ops (include/gftaylor.h states the loops) ----------------------------------------------------------------


def derivative(x, var, k, out=None):
    """The ``k``-th derivative in variable ``var`` (0: axis -2, 1: axis -1): slice ``j`` of the result is slice ``k + j`` of ``x`` times
    the reference's factor ``ff_j`` (``series.derivative``), one rounding per coefficient; the axis is ``k`` shorter."""
    return _run(_CALL, "derivative", x, out=out, scalar=k, var=var)


def taylor_expansion_of_coeff(x, var, k, out=None):
    """The expansion of the coefficient of ``var**k``: slice 0 is slice ``k`` of ``x`` untouched, slice ``j >= 1`` is slice ``k + j``
    times ``f_j`` (``series.taylor_expansion_of_coeff``)."""
    return _run(_CALL, "taylor_expansion_of_coeff", x, out=out, scalar=k, var=var)


def shift_down(x, var, k, out=None):
    """Variable ``var`` moved down by ``k``: slice 0 of the result is slice ``k`` of ``x`` plus the ordered sum of slices ``0 .. k-1``
    (all slices when the axis has ``k + 1``), the others are copies.  The order is ndarray's ``sum_axis``: along axis -2 ascending over
    the rows from 0.0 per column; along axis -1, and along axis -2 of a one-column item, the 8-way unrolled fold."""
    return _run(_CALL, "shift_down", x, out=out, scalar=k, var=var)


def evaluate_all_one(x, out=None):
    """Every item at ``(1, 1)``: ``0.0 + x[b, 0, 0] + x[b, 0, 1] + ...`` in row-major order, one chain; the batch shape."""
    return _run(_CALL, "evaluate_all_one", x, out=out)


def observe_chain(a, var, x, cs, degree_p1=None, out=None):
    """``series.observe_chain`` along variable ``var`` (0: axis -2, 1: axis -1) of every item: each line along that axis runs the
    chain, the other axis is cut to ``min(len, degree_p1)`` and carried along.  The result has ``degree_p1`` coefficients on the axis of
    ``var`` (default: its stored length less ``nsteps``).  ``x``: the batch shape or ``None`` (continuous rate); ``cs``: ``[B..., nsteps]``."""
    from ._series_call import run_chain

    return run_chain(_CALL, a, var, x, cs, degree_p1, out)


def observe_negbinomial(a, var, x, p, ls, degree_p1=None, out=None):
    """``series.observe_negbinomial`` along variable ``var`` (0: axis -2, 1: axis -1) of every item: each line along that axis runs the
    passes, the other axis is cut to ``min(len, degree_p1)``.  The row comes from ``series.lah_row``."""
    from ._series_call import run_negbinomial

    return run_negbinomial(_CALL, a, var, x, p, ls, degree_p1, out)


def mul_linear(a, var, c, m, n=None, out=None):
    """``a`` times the linear series ``c + m * x_var`` (``var`` 0: axis -2, 1: axis -1): ``series.mul_linear`` on every line along that
    axis.  ``n`` (default: ``a``'s shape with one more on the axis) is the result's order, a pair."""
    from ._series_call import run_linear

    return run_linear(_CALL, "mul_linear", a, var, None, c, m, n, out)


def compose_linear(f, var, c, m, wvar=None, n=None, out=None):
    """``f`` with ``x_var := c + m * x_wvar`` (``wvar`` defaults to ``var``).  ``wvar == var``: ``series.compose_linear`` on every line
    along the axis.  Otherwise the slices of ``f`` along ``var`` are the Horner coefficients and the result keeps index 0 alone on that
    axis.  ``n`` (default: the stored shape of the result, with ``f``'s own length on ``var`` where ``wvar != var``) is the result's order,
    a pair."""
    from ._series_call import run_linear

    return run_linear(_CALL, "compose_linear", f, var, wvar, c, m, n, out)
