"""Batched univariate series on float64 device tensors: ``mul``, ``div``, ``exp``, ``log``, ``compose``, ``pow`` (``gft_series_*``).

The last axis of every tensor is the series (coefficient ``k`` of ``t^k`` at index ``k``, unit stride), the leading axes are
batch axes and broadcast by torch's rules (``expand``, no copy: one series against a whole batch has batch stride 0).
Item ``b`` is the ``TaylorPoly<F64>`` of one variable with stored coefficients ``x[b, :nx]`` and truncation order ``n``; a
tensor shorter than ``n`` is a compact operand.  Per item the results are the reference's *general* algorithms in its
operation order — none of the shortcuts the handle operators take on zero / one / constant / linear operands, so a result
never depends on what else is in the batch.  The call is ordered on torch's current stream and does not wait.

    >>> from genfer_amd import series
    >>> z = series.mul(x, y)             # x, y: [B, n] float64 on the GPU
    >>> q = series.div(x, y[0])          # every row by one series
    >>> e = series.exp(x, seed=torch.exp(x[..., 0]))
    >>> h = series.compose(f, g)         # f(g(t)) per item: Horner over f's coefficients, one launch
    >>> p = series.pow(x, 5)             # square-and-multiply over mul

``compose`` costs about ``nf * n**2 / 2`` multiply-adds per item and a series never leaves its one workgroup (the Horner steps
are a dependency chain), so a few long series are slow by construction; no cap is imposed.
"""
from __future__ import annotations

import ctypes as C

from .taylor import TaylorError

MAX_N = 4096  # gft_series.hpp SERIES_MAX_N: the limit of this version

_declared = None


def _lib():
    global _declared
    if _declared is None:
        from . import lib

        L = lib()
        i64, sz, vp = C.POINTER(C.c_int64), C.POINTER(C.c_size_t), C.c_void_p
        for pre in ("gft_series_", "gfti_series_"):  # the interval twins (interval_series.py) take the same argument lists
            for name in ("mul", "div", "compose"):
                f = getattr(L, pre + name)
                f.restype, f.argtypes = C.c_int, [vp, i64, C.c_size_t, vp, i64, C.c_size_t, vp, i64, C.c_size_t, sz, C.c_size_t, vp]
            for name in ("exp", "log"):
                f = getattr(L, pre + name)
                f.restype, f.argtypes = C.c_int, [vp, i64, C.c_size_t, vp, i64, vp, i64, C.c_size_t, sz, C.c_size_t, vp]
            f = getattr(L, pre + "pow")
            f.restype, f.argtypes = C.c_int, [vp, i64, C.c_size_t, C.c_uint32, vp, i64, C.c_size_t, sz, C.c_size_t, vp]
        L.gft_series_last_form.restype, L.gft_series_last_form.argtypes = C.c_int, []
        _declared = L
    return _declared


def _check(torch, t, what, series_axis=True, planes=0):
    """Everything that can be refused without the library: type, dtype, placement, the series axis (and, for an interval
    tensor, the leading axis of the two planes)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float64:
        raise TaylorError(f"{what}: the tensor is {t.dtype}; only torch.float64 is accepted (no implicit conversion)")
    if t.device.type != "cuda":
        raise TaylorError(f"{what}: the tensor is on {t.device}; it must be in device memory of the library's GPU")
    if planes and (t.dim() < 1 or t.shape[0] != 2):
        lead = "no axes" if t.dim() < 1 else f"a first axis of {t.shape[0]}"
        raise TaylorError(f"{what}: the tensor has {lead}; an interval tensor is stacked [2, ...] = (lo, hi) along its first axis")
    if series_axis:
        if t.dim() < 1 + planes:
            raise TaylorError(f"{what}: a 0-dimensional tensor has no series axis")
        if t.shape[-1] > 1 and t.stride(-1) != 1:
            raise TaylorError(f"{what}: the series (last) axis has stride {t.stride(-1)}; it must have unit stride")
        if t.shape[-1] == 0:
            raise TaylorError(f"{what}: the series (last) axis is empty")


def _order(what, n, *lens, max_n=None):
    max_n = MAX_N if max_n is None else max_n
    if n is None:
        n = max(lens)
    n = int(n)
    if n < 1:
        raise TaylorError(f"{what}: n = {n}; the result needs at least one coefficient (n == 0 is refused)")
    if n > max_n:
        raise TaylorError(f"{what}: n = {n} exceeds the limit of {max_n} coefficients per series of this version")
    for ln in lens:
        if ln > n:
            raise TaylorError(f"{what}: an operand has {ln} coefficients, more than n = {n} (nx > n)")
    return n


def _i64(seq):
    seq = [int(s) for s in seq]
    return (C.c_int64 * max(len(seq), 1))(*seq)


def _run(what, fn_name, x, second, n, out, second_is_seed, names=("x", "y"), e=None, planes=0, max_n=None):
    """One call of either family.  planes = 1: the tensors are interval tensors [2, B..., n] (seeds [2, B...]); the leading
    axis travels as the first entry of every stride array, which is where the gfti_series_* entry points expect it."""
    import torch

    _check(torch, x, f"{what}: {names[0]}", planes=planes)
    if second is not None:
        _check(torch, second, f"{what}: {'seed' if second_is_seed else names[1]}", series_axis=not second_is_seed, planes=planes)
    if out is not None:
        _check(torch, out, f"{what}: out", planes=planes)
    lens = (x.shape[-1],) if second_is_seed or second is None else (x.shape[-1], second.shape[-1])
    n = _order(what, n, *lens, max_n=max_n)
    for t in (second, out):
        if t is not None and t.device != x.device:
            raise TaylorError(f"{what}: the tensors are on different devices ({x.device}, {t.device})")
    lead = (2,) * planes
    shapes = [x.shape[planes:-1]]
    if second is not None:
        shapes.append(second.shape[planes:] if second_is_seed else second.shape[planes:-1])
    if out is not None:
        if out.shape[-1] != n:
            raise TaylorError(f"{what}: out has {out.shape[-1]} coefficients per series, the result has n = {n}")
        batch = tuple(out.shape[planes:-1])
        if tuple(torch.broadcast_shapes(*shapes, batch)) != batch:
            raise TaylorError(f"{what}: out has batch shape {batch}; the operands broadcast to {tuple(torch.broadcast_shapes(*shapes))}")
    else:
        batch = tuple(torch.broadcast_shapes(*shapes))
        out = torch.empty(lead + batch + (n,), dtype=torch.float64, device=x.device)
    if planes:  # torch aligns shapes from the right: the plane axis stays first, missing batch axes go behind it (a view)
        lift = lambda t, rank: t if t.dim() >= rank else t[(slice(None),) + (None,) * (rank - t.dim())]  # noqa: E731
        x = lift(x, len(batch) + 2)
        if second is not None:
            second = lift(second, len(batch) + (1 if second_is_seed else 2))
    L = _lib()
    dev = int(L.gft_device())
    if dev >= 0 and x.device.index != dev:
        raise TaylorError(f"{what}: the tensors are on {x.device}, but the library runs on cuda:{dev}")
    xe = x.expand(lead + batch + (x.shape[-1],))
    nb = len(batch)
    ns = nb + planes  # entries of a stride array
    bsz = (C.c_size_t * max(nb, 1))(*batch)
    stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    fn = getattr(L, fn_name)
    if e is not None:
        rc = fn(C.c_void_p(xe.data_ptr()), _i64(xe.stride()[:ns]), xe.shape[-1], e, C.c_void_p(out.data_ptr()), _i64(out.stride()[:ns]),
                n, bsz, nb, stream)
    elif second_is_seed:
        if second is None:
            sp, sbs = None, None
        else:
            se = second.expand(lead + batch)
            sp, sbs = C.c_void_p(se.data_ptr()), _i64(se.stride())
        rc = fn(C.c_void_p(xe.data_ptr()), _i64(xe.stride()[:ns]), xe.shape[-1], sp, sbs, C.c_void_p(out.data_ptr()),
                _i64(out.stride()[:ns]), n, bsz, nb, stream)
    else:
        ye = second.expand(lead + batch + (second.shape[-1],))
        rc = fn(C.c_void_p(xe.data_ptr()), _i64(xe.stride()[:ns]), xe.shape[-1], C.c_void_p(ye.data_ptr()), _i64(ye.stride()[:ns]),
                ye.shape[-1], C.c_void_p(out.data_ptr()), _i64(out.stride()[:ns]), n, bsz, nb, stream)
    if rc != 0:
        raise TaylorError((L.gft_last_error() or b"unknown error").decode())
    return out


def mul(x, y, n=None, out=None):
    """``z[b] = x[b] * y[b]`` truncated at order ``n`` (default ``max(nx, ny)``): the general product ``mul_1d``."""
    return _run("series.mul", "gft_series_mul", x, y, n, out, False)


def div(x, y, n=None, out=None):
    """``r[b] = x[b] / y[b]`` to order ``n`` (default ``max(nx, ny)``): the general division recurrence."""
    return _run("series.div", "gft_series_div", x, y, n, out, False)


def exp(x, n=None, seed=None, out=None):
    """``exp(x[b])`` to order ``n`` (default ``nx``).  ``seed``: ``exp(x[b, 0])`` per item (a tensor of the batch shape); with
    the host libm's values the result carries the reference's bits.  ``None``: formed on the device (a few ulps from libm)."""
    return _run("series.exp", "gft_series_exp", x, seed, n, out, True)


def log(x, n=None, seed=None, out=None):
    """``log(x[b])`` to order ``n`` (default ``nx``).  ``seed``: ``ln(x[b, 0])`` per item; ``None``: formed on the device (only
    coefficient 0 depends on it)."""
    return _run("series.log", "gft_series_log", x, seed, n, out, True)


def compose(f, g, n=None, out=None):
    """``f[b](g[b])`` truncated at order ``n`` (default ``max(nf, ng)``): Horner over the coefficients of ``f`` with the general
    product at every step, ``res = res * g + f[i]`` for ``i = nf-2 .. 0`` from ``res = [0.0 + f[nf-1]]`` — ``subst_var``'s general
    path without its zero / linear shortcuts, the row resident in LDS across the steps.  About ``nf * n**2 / 2`` multiply-adds per
    item, on one workgroup at most."""
    return _run("series.compose", "gft_series_compose", f, g, n, out, False, names=("f", "g"))


def _exponent(what, e, div="series.div"):
    """pow's exponent, judged before anything else (shared with interval_series.pow)"""
    import operator

    if isinstance(e, bool):
        raise TypeError(f"{what}: e must be a non-negative integer, got a bool")
    try:
        ei = operator.index(e)
    except TypeError:
        raise TypeError(f"{what}: e must be a non-negative integer, got {e!r} (a non-integral exponent is not a series power)") from None
    if ei < 0:
        raise TaylorError(f"{what}: e = {ei} is negative (use {div} for reciprocals)")
    if ei >= 2**32:
        raise TaylorError(f"{what}: e = {ei} does not fit the 32 bits of the exponent")
    return ei


def pow(x, e, n=None, out=None):  # noqa: A001 (the reference's name)
    """``x[b] ** e`` truncated at order ``n`` (default ``nx``) for an integer ``0 <= e < 2**32``: the reference's
    square-and-multiply over ``mul`` at compact lengths.  ``e = 0`` gives ``[1, 0, ...]``."""
    return _run("series.pow", "gft_series_pow", x, None, n, out, True, e=_exponent("series.pow", e))


FORMS = {0: None, 1: "A", 2: "B"}


def last_form():
    """Which form the last call took: "A" (one lane per series), "B" (one wave / workgroup per series) or None."""
    return FORMS[int(_lib().gft_series_last_form())]


def set_form(form=None):
    """Ask for a form ("A" holds only where the rows fit its LDS budget), or None for the library's thresholds.  For tests
    and measurements."""
    v = {None: 0.0, "A": 1.0, "B": 2.0}[form]
    if _lib().gft_set_option(b"series_form", v) != 0:
        raise TaylorError("series.set_form: the library does not know the option")
