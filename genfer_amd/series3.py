"""Batched trivariate series on float64 device tensors: ``mul``, ``div``, ``exp``, ``log``, ``compose``, ``pow`` (``gft_series3_*``).

The last three axes of every tensor are the coefficient array of one ``TaylorPoly<F64>`` in three variables: axis -3 is variable 0
(the slabs) and axis -2 variable 1 (the rows), both with any non-negative stride; axis -1 is variable 2 (unit stride).  The leading
axes are batch axes and broadcast by torch's rules (``expand``, no copy).  An operand of stored shape ``(nx0, nx1, nx2)`` smaller
than the result's ``n = (n0, n1, n2)`` is a compact operand.  Per item the results are the reference's *general* recursion over
axis 0 in its operation order -- none of the shortcuts the handle operators take, so a result never depends on what else is in the
batch -- computed, as the reference does, at the stored result shape ``S`` that follows from the shapes alone (``mul``:
``min(n, nx + ny - 1)`` per axis; ``div``: ``n``, but ``nx`` where ``y`` has one coefficient; ``exp`` / ``log``: ``n``, but 1 where
``x`` has one).  Everything outside ``S`` is ``+0.0``, and an ``S`` with unit axes is the ``series2`` item (the ``series`` row, the
scalar) without them.  ``include/gftaylor.h`` states the loops.  One launch per call, one workgroup per item;
``n0 * n1 * n2 <= 4096``.  The call is ordered on torch's current stream and does not wait.  ``compose`` substitutes a series for
one of the three variables (``subst_var``'s Horner loop over ``mul``'s product, the whole loop in one launch); ``pow`` is
square-and-multiply over ``mul``'s launches inside one call.

    >>> from genfer_amd import series3
    >>> z = series3.mul(x, y)                      # x, y: [B, n0, n1, n2] float64 on the GPU
    >>> q = series3.div(x, y[0])                   # every item by one series
    >>> e = series3.exp(x, seed=torch.exp(x[..., 0, 0, 0]))
    >>> h = series3.compose(f, g, var=2)           # g for variable 2 (axis -1) of f
    >>> p = series3.pow(x, 5)

No autograd: this is the raw layer, and an operand that requires grad is refused while grad mode is on (``detach()`` it, or use
``torch.no_grad()``).  float64 only.
"""
from __future__ import annotations

from ._series_call import Call
from ._series_call import run as _run
from .series import _exponent
from .taylor import TaylorError

MAX_ELEMS = 4096  # gft_series_args.hpp SERIES3_MAX_ELEMS: n0 * n1 * n2 of the result in this version

_CALL = Call("series3", 3, 0, MAX_ELEMS, raw=True)  # rank 3, one plane, no autograd


def _orders(what, n, *shapes, max_elems=None):
    max_elems = MAX_ELEMS if max_elems is None else max_elems
    if n is None:
        n = tuple(max(s[a] for s in shapes) for a in range(3))
    try:
        n0, n1, n2 = (int(v) for v in n)
    except (TypeError, ValueError):
        raise TypeError(f"{what}: n must be a triple (n0, n1, n2), got {n!r}") from None
    n = (n0, n1, n2)
    if min(n) < 1:
        raise TaylorError(f"{what}: n = {n}; the result needs at least one coefficient on each axis (n == 0 is refused)")
    if n0 * n1 * n2 > max_elems:
        raise TaylorError(f"{what}: n0 * n1 * n2 = {n0} * {n1} * {n2} = {n0 * n1 * n2} exceeds the limit of {max_elems} coefficients per item "
                          "of this version")
    for s in shapes:
        for a in range(3):
            if s[a] > n[a]:
                raise TaylorError(f"{what}: an operand has {s[a]} coefficients on axis {a - 3}, more than n{a} = {n[a]} (nx > n)")
    return n


def mul(x, y, n=None, out=None):
    """``z[b] = x[b] * y[b]`` truncated at orders ``n = (n0, n1, n2)`` (default: the larger stored length on each axis)."""
    return _run(_CALL, "mul", x, y, n, out)


def div(x, y, n=None, out=None):
    """``r[b] = x[b] / y[b]`` to orders ``n``: the general division recurrence over the slabs, every slab step the rank-2
    division of ``series2.div``."""
    return _run(_CALL, "div", x, y, n, out)


def exp(x, n=None, seed=None, out=None):
    """``exp(x[b])`` to orders ``n``.  ``seed``: ``exp(x[b, 0, 0, 0])`` per item (a tensor of the batch shape); with the host
    libm's values the result carries the reference's bits.  ``None``: formed on the device (a few ulps from libm)."""
    return _run(_CALL, "exp", x, seed, n, out)


def log(x, n=None, seed=None, out=None):
    """``log(x[b])`` to orders ``n``.  ``seed``: ``ln(x[b, 0, 0, 0])`` per item; ``None``: formed on the device (only coefficient
    ``[0, 0, 0]`` depends on it)."""
    return _run(_CALL, "log", x, seed, n, out)


def _var(what, var):
    """compose's variable: 0 (axis -3), 1 (axis -2) or 2 (axis -1)"""
    if isinstance(var, bool) or not isinstance(var, int) or var not in (0, 1, 2):
        raise TaylorError(f"{what}: var = {var!r}; the variable of f that g replaces is 0 (axis -3), 1 (axis -2) or 2 (axis -1)")
    return var


def compose(f, g, var=0, n=None, out=None):
    """``f[b]`` with ``g[b]`` substituted for variable ``var`` (0: axis -3, 1: axis -2, 2: axis -1) of ``f``, truncated at
    ``n = (n0, n1, n2)`` (default: the larger stored length on each axis).  ``subst_var``'s general Horner path without its
    shortcuts: over the slices of ``f`` along the substituted axis, ``res = mul(res, g) + slice`` with ``mul``'s product -- its stored
    shape and its squeeze included -- at the compact shape ``min(r + ng - 1, n)`` of every step, from ``res = 0.0 + the last slice``;
    the result stays in LDS across the steps of the one launch.  With one slice the result is ``0.0 + f`` and ``g``'s values are not
    read.  ``out`` may be ``f`` or ``g`` itself.  Cost: about ``nslices * (n0*n1*n2)**2 / 8`` multiply-adds per item, all on one
    workgroup; no cap is imposed."""
    return _run(_CALL, "compose", f, g, n, out, var=_var("series3.compose", var))


def pow(x, e, n=None, out=None):  # noqa: A001 (the reference's name)
    """``x[b] ** e`` truncated at ``n = (n0, n1, n2)`` (default: the stored shape) for an integer ``0 <= e < 2**32``: the reference's
    square-and-multiply over ``mul`` at compact shapes.  ``e = 0`` gives the unit item (1.0 at ``[0, 0, 0]``); ``e = 1`` runs the
    loop, ``0.0 + 1.0 * x``.  ``out`` may be ``x`` itself."""
    e = _exponent("series3.pow", e, div="series3.div")
    return _run(_CALL, "pow", x, None, n, out, scalar=e)
