"""Batched bivariate series on float64 device tensors: ``mul``, ``div``, ``exp``, ``log``, ``compose``, ``pow`` and the transposed
product ``corr`` and the observation ops ``derivative``, ``taylor_expansion_of_coeff``, ``shift_down``, ``evaluate_all_one``
(``gft_series2_*``).

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

import ctypes as C

from .series import _check, _exponent, _i64, _observe, _placed
from .taylor import TaylorError

MAX_ELEMS = 4096  # gft_series.hpp SERIES2_MAX_ELEMS: n0 * n1 of the result in this version

_declared = None


def _lib():
    global _declared
    if _declared is None:
        from . import lib

        L = lib()
        i64, sz, vp, i, s = C.POINTER(C.c_int64), C.POINTER(C.c_size_t), C.c_void_p, C.c_int64, C.c_size_t
        for pre in ("gft_series2_", "gfti_series2_"):  # the interval twins (interval_series2.py) take the same argument lists
            for name in ("mul", "div"):
                f = getattr(L, pre + name)
                f.restype, f.argtypes = C.c_int, [vp, i64, i, s, s, vp, i64, i, s, s, vp, i64, i, s, s, sz, s, vp]
            for name in ("exp", "log"):
                f = getattr(L, pre + name)
                f.restype, f.argtypes = C.c_int, [vp, i64, i, s, s, vp, i64, vp, i64, i, s, s, sz, s, vp]
            f = getattr(L, pre + "compose")
            f.restype, f.argtypes = C.c_int, [vp, i64, i, s, s, vp, i64, i, s, s, C.c_int, vp, i64, i, s, s, sz, s, vp]
            f = getattr(L, pre + "pow")
            f.restype, f.argtypes = C.c_int, [vp, i64, i, s, s, C.c_uint32, vp, i64, i, s, s, sz, s, vp]
            for name in ("derivative", "taylor_expansion_of_coeff", "shift_down"):  # the observation ops: x, var, k, the result
                f = getattr(L, pre + name)
                f.restype, f.argtypes = C.c_int, [vp, i64, i, s, s, C.c_int, s, vp, i64, i, s, s, sz, s, vp]
            f = getattr(L, pre + "evaluate_all_one")
            f.restype, f.argtypes = C.c_int, [vp, i64, i, s, s, vp, i64, sz, s, vp]
        # the transposed operations (f64 only): mul's and compose's argument lists
        L.gft_series2_corr.restype, L.gft_series2_corr.argtypes = C.c_int, [vp, i64, i, s, s, vp, i64, i, s, s, vp, i64, i, s, s, sz, s, vp]
        f = L.gft_series2_compose_adj
        f.restype, f.argtypes = C.c_int, [vp, i64, i, s, s, vp, i64, i, s, s, C.c_int, vp, i64, i, s, s, sz, s, vp]
        L.gft_series_last_form.restype, L.gft_series_last_form.argtypes = C.c_int, []
        _declared = L
    return _declared


def _axes(t, what, planes=0):
    """the two series axes of an operand or of ``out`` (type and dtype are judged by series._check)"""
    if t.dim() < 2 + planes:
        if planes:
            raise TaylorError(f"{what}: the tensor has {t.dim()} axes; a bivariate interval series needs at least 3 (the first holds the two "
                              "planes, the last two are the coefficient array)")
        raise TaylorError(f"{what}: the tensor has {t.dim()} axes; a bivariate series needs at least 2 (the last two are the coefficient array)")
    if t.shape[-1] == 0 or t.shape[-2] == 0:
        raise TaylorError(f"{what}: a series axis is empty (the last two axes are {tuple(t.shape[-2:])})")
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        raise TaylorError(f"{what}: the series (last) axis has stride {t.stride(-1)}; it must have unit stride")


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


def _run(what, fn_name, x, second, n, out, second_is_seed, names=("x", "y"), scalar=None, planes=0, max_elems=None, short=False):
    """``scalar``: compose's ``var`` (passed behind the second operand) or pow's ``e`` (in the place of the seeds).  planes = 1:
    the tensors are interval tensors [2, B..., n0, n1] (seeds [2, B...]); the leading axis travels as the first entry of every
    batch-stride array, which is where the gfti_series2_* entry points expect it.  short: a transposed operation (corr,
    _compose_adj), whose result is no larger than its first operand; names[2] names it."""
    import torch

    # everything that needs no device first: types, shapes, strides, orders, out, grad -- then the placement
    xname = names[0]
    _check(torch, x, f"{what}: {xname}", series_axis=False, planes=planes, placement=False)
    _axes(x, f"{what}: {xname}", planes)
    sname = "seed" if second_is_seed else names[1]
    if second is not None:
        _check(torch, second, f"{what}: {sname}", series_axis=False, planes=planes, placement=False)
        if not second_is_seed:
            _axes(second, f"{what}: {sname}", planes)
    if out is not None:
        _check(torch, out, f"{what}: out", series_axis=False, planes=planes, placement=False)
        _axes(out, f"{what}: out", planes)
    operands = [x] if second_is_seed or second is None else [x, second]
    if short:
        n0, n1 = _orders_short(what, n, *(tuple(t.shape[-2:]) for t in operands), names)
    else:
        n0, n1 = _orders(what, n, *(tuple(t.shape[-2:]) for t in operands), max_elems=max_elems)
    lead = (2,) * planes
    shapes = [x.shape[planes:-2]]
    if second is not None:
        shapes.append(second.shape[planes:] if second_is_seed else second.shape[planes:-2])
    if out is not None:
        if tuple(out.shape[-2:]) != (n0, n1):
            raise TaylorError(f"{what}: out has {tuple(out.shape[-2:])} coefficients per item, the result has n = ({n0}, {n1})")
        batch = tuple(out.shape[planes:-2])
        if tuple(torch.broadcast_shapes(*shapes, batch)) != batch:
            raise TaylorError(f"{what}: out has batch shape {batch}; the operands broadcast to {tuple(torch.broadcast_shapes(*shapes))}")
    else:
        batch = tuple(torch.broadcast_shapes(*shapes))
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, second)):
        mod = what.split(".")[0]
        raise TaylorError(f"{what}: an operand requires grad, and this version of {mod} has no autograd; pass {xname}.detach() or call under "
                          "torch.no_grad() (nothing is detached silently)")
    _placed(x, f"{what}: {xname}")
    if second is not None:
        _placed(second, f"{what}: {sname}")
    if out is not None:
        _placed(out, f"{what}: out")
    for t in (second, out):
        if t is not None and t.device != x.device:
            raise TaylorError(f"{what}: the tensors are on different devices ({x.device}, {t.device})")
    if out is None:
        out = torch.empty(lead + batch + (n0, n1), dtype=torch.float64, device=x.device)
    nb = len(batch)
    if planes:  # torch aligns shapes from the right: the plane axis stays first, missing batch axes go behind it (a view)
        lift = lambda t, rank: t if t.dim() >= rank else t[(slice(None),) + (None,) * (rank - t.dim())]  # noqa: E731
        x = lift(x, nb + 3)
        if second is not None:
            second = lift(second, nb + (1 if second_is_seed else 3))
    L = _lib()
    dev = int(L.gft_device())
    if dev >= 0 and x.device.index != dev:
        raise TaylorError(f"{what}: the tensors are on {x.device}, but the library runs on cuda:{dev}")
    ns = nb + planes  # entries of a batch-stride array
    xe = x.expand(lead + batch + tuple(x.shape[-2:]))
    bsz = (C.c_size_t * max(nb, 1))(*batch)
    stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    fn = getattr(L, fn_name)
    xa = (C.c_void_p(xe.data_ptr()), _i64(xe.stride()[:ns]), xe.stride(-2), xe.shape[-2], xe.shape[-1])
    ra = (C.c_void_p(out.data_ptr()), _i64(out.stride()[:ns]), out.stride(-2), n0, n1, bsz, nb, stream)
    if second_is_seed:
        if scalar is not None:
            sa = (C.c_uint32(scalar),)
        elif second is None:
            sa = (None, None)
        else:
            se = second.expand(lead + batch)
            sa = (C.c_void_p(se.data_ptr()), _i64(se.stride()))
        rc = fn(*xa, *sa, *ra)
    else:
        ye = second.expand(lead + batch + tuple(second.shape[-2:]))
        va = () if scalar is None else (C.c_int(scalar),)
        rc = fn(*xa, C.c_void_p(ye.data_ptr()), _i64(ye.stride()[:ns]), ye.stride(-2), ye.shape[-2], ye.shape[-1], *va, *ra)
    if rc != 0:
        raise TaylorError((L.gft_last_error() or b"unknown error").decode())
    return out


def mul(x, y, n=None, out=None):
    """``z[b] = x[b] * y[b]`` truncated at orders ``n = (n0, n1)`` (default: the larger stored length on each axis)."""
    return _run("series2.mul", "gft_series2_mul", x, y, n, out, False)


def div(x, y, n=None, out=None):
    """``r[b] = x[b] / y[b]`` to orders ``n = (n0, n1)``: the general division recurrence over the rows."""
    return _run("series2.div", "gft_series2_div", x, y, n, out, False)


def exp(x, n=None, seed=None, out=None):
    """``exp(x[b])`` to orders ``n``.  ``seed``: ``exp(x[b, 0, 0])`` per item (a tensor of the batch shape); with the host libm's
    values the result carries the reference's bits.  ``None``: formed on the device (a few ulps from libm)."""
    return _run("series2.exp", "gft_series2_exp", x, seed, n, out, True)


def log(x, n=None, seed=None, out=None):
    """``log(x[b])`` to orders ``n``.  ``seed``: ``ln(x[b, 0, 0])`` per item; ``None``: formed on the device (only coefficient
    ``[0, 0]`` depends on it)."""
    return _run("series2.log", "gft_series2_log", x, seed, n, out, True)


def compose(f, g, var=0, n=None, out=None):
    """``f[b]`` with ``g[b]`` substituted for variable ``var`` (0: axis -2, 1: axis -1) of ``f``, truncated at ``n = (n0, n1)``
    (default: the larger stored length on each axis).  ``subst_var``'s general Horner path without its shortcuts: over the slices
    of ``f`` along the substituted axis, ``res = res * g + slice`` with the general product at the compact shape of every step,
    from ``res = 0.0 + the last slice``; the result stays in LDS across the steps of the one launch.  Cost: about
    ``nslices * (n0*n1)**2 / 4`` multiply-adds per item, all on one workgroup; no cap is imposed."""
    if isinstance(var, bool) or not isinstance(var, int) or var not in (0, 1):
        raise TaylorError(f"series2.compose: var = {var!r}; the variable of f that g replaces is 0 or 1")
    return _run("series2.compose", "gft_series2_compose", f, g, n, out, False, names=("f", "g"), scalar=var)


def _var(what, var):
    if isinstance(var, bool) or not isinstance(var, int) or var not in (0, 1):
        raise TaylorError(f"{what}: var = {var!r}; the variable of f that g replaces is 0 or 1")
    return var


def corr(g, y, m=None, out=None):
    """The transposed product, the adjoint of ``mul``: ``<mul(x, y, g.shape), g> = <x, corr(g, y)>``.  ``g`` has stored shape
    ``(g0, g1)`` with ``g0 * g1 <= 4096``, ``y`` has ``(ny0, ny1) <= (g0, g1)`` per axis, the result ``m = (m0, m1) <= (g0, g1)``
    per axis (default: ``g``'s stored shape)::

        c[b, i0, i1] = 0.0 + sum_k0 (0.0 + sum_k1 g[b, k0, k1] * y[b, k0 - i0, k1 - i1])

    with ``k0`` descending from ``min(g0 - 1, i0 + ny0 - 1)`` to ``i0`` and ``k1`` from ``min(g1 - 1, i1 + ny1 - 1)`` to ``i1``,
    multiply and add rounded separately, only stored coefficients entering a sum: bit for bit ``mul(flip(g), y, n=g.shape)`` at
    index ``[g0 - 1 - i0, g1 - 1 - i1]``, ``flip`` reversing both series axes.  ``out`` may be ``g`` itself, never ``y``."""
    return _run("series2.corr", "gft_series2_corr", g, y, m, out, False, names=("g", "y", "m"), short=True)


def _compose_adj(gh, g, var, nf, out=None):
    """The transposed Horner loop: the gradient of ``compose(f, g, var, n)`` with respect to ``f`` (stored shape ``nf``) from the
    gradient ``gh`` of the composition (shape ``n``).  With ``S`` slices of ``f`` of ``len`` coefficients along axis ``var`` and
    ``L_i = min(base + (S - 1 - i) * (ng - 1), n)`` per axis, ``base = (1, len)`` / ``(len, 1)``: ``a = gh[:L_0]``; slice ``i`` of the
    result is the first ``len`` entries of row 0 (var 0) / column 0 (var 1) of ``a``; then ``a = corr(a, g, L_{i+1})`` -- in one launch."""
    _var("series2._compose_adj", var)
    return _run("series2._compose_adj", "gft_series2_compose_adj", gh, g, nf, out, False, names=("gh", "g", "nf"), scalar=var, short=True)


def pow(x, e, n=None, out=None):  # noqa: A001 (the reference's name)
    """``x[b] ** e`` truncated at ``n = (n0, n1)`` (default: the stored shape) for an integer ``0 <= e < 2**32``: the reference's
    square-and-multiply over ``mul`` at compact shapes.  ``e = 0`` gives the unit item ``[[1, 0, ...], [0, ...], ...]``."""
    e = _exponent("series2.pow", e, div="series2.div")
    return _run("series2.pow", "gft_series2_pow", x, None, n, out, True, scalar=e)


# ---- the observation ops (series._observe at rank 2; include/gftaylor.h states the loops) -------------------------------------


def derivative(x, var, k, out=None):
    """The ``k``-th derivative in variable ``var`` (0: axis -2, 1: axis -1): slice ``j`` of the result is slice ``k + j`` of ``x`` times
    the reference's factor ``ff_j`` (``series.derivative``), one rounding per coefficient; the axis is ``k`` shorter."""
    return _observe("series2.derivative", "derivative", x, k, out, rank=2, var=var, limit=MAX_ELEMS, raw=True)


def taylor_expansion_of_coeff(x, var, k, out=None):
    """The expansion of the coefficient of ``var**k``: slice 0 is slice ``k`` of ``x`` untouched, slice ``j >= 1`` is slice ``k + j``
    times ``f_j`` (``series.taylor_expansion_of_coeff``)."""
    return _observe("series2.taylor_expansion_of_coeff", "taylor_expansion_of_coeff", x, k, out, rank=2, var=var, limit=MAX_ELEMS, raw=True)


def shift_down(x, var, k, out=None):
    """Variable ``var`` moved down by ``k``: slice 0 of the result is slice ``k`` of ``x`` plus the ordered sum of slices ``0 .. k-1``
    (all slices when the axis has ``k + 1``), the others are copies.  The order is ndarray's ``sum_axis``: along axis -2 ascending over
    the rows from 0.0 per column; along axis -1, and along axis -2 of a one-column item, the 8-way unrolled fold."""
    return _observe("series2.shift_down", "shift_down", x, k, out, rank=2, var=var, limit=MAX_ELEMS, raw=True)


def evaluate_all_one(x, out=None):
    """Every item at ``(1, 1)``: ``0.0 + x[b, 0, 0] + x[b, 0, 1] + ...`` in row-major order, one chain; the batch shape."""
    return _observe("series2.evaluate_all_one", "evaluate_all_one", x, None, out, rank=2, limit=MAX_ELEMS, raw=True)
