"""Batched univariate series on float64 device tensors: ``mul``, ``div``, ``exp``, ``log``, ``compose``, ``pow``, the transposed
product ``corr`` and the observation ops ``derivative``, ``taylor_expansion_of_coeff``, ``shift_down``, ``evaluate_all_one``
(``gft_series_*``), all but ``corr`` differentiable by torch's autograd.

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
    >>> d = series.derivative(h, 2)      # [B, n - 2]: h[b, 2 + j] times the reference's factor table
    >>> m = series.evaluate_all_one(h)   # [B]: 0.0 + h[b, 0] + h[b, 1] + ..., the reference's order

Gradients: when grad mode is on and an operand has ``requires_grad=True`` the six operations record a ``grad_fn`` (forward values
are the same bits either way).  Every backward pass is a short sequence of calls of this module around ``corr``, the adjoint of the
truncated product, ``<mul(x, y), g> = <x, corr(g, y)>``; ``compose`` adds one kernel, the transposed Horner loop.  First derivatives
only (``once_differentiable``), float64 only; ``out=`` cannot be combined with an operand that requires grad, and a ``seed`` never
carries a gradient (it is ``exp(x[..., 0])`` / ``ln(x[..., 0])`` by contract: the gradient flows to ``x``).

    >>> w = torch.rand(8, dtype=torch.float64, device="cuda", requires_grad=True)
    >>> series.compose(w, g).sum().backward()   # w.grad: one launch of the transposed Horner loop, summed over the batch

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
            for name in ("mul", "div", "compose") + (("corr", "compose_adj") if pre == "gft_series_" else ()):
                f = getattr(L, pre + name)
                f.restype, f.argtypes = C.c_int, [vp, i64, C.c_size_t, vp, i64, C.c_size_t, vp, i64, C.c_size_t, sz, C.c_size_t, vp]
            for name in ("exp", "log"):
                f = getattr(L, pre + name)
                f.restype, f.argtypes = C.c_int, [vp, i64, C.c_size_t, vp, i64, vp, i64, C.c_size_t, sz, C.c_size_t, vp]
            f = getattr(L, pre + "pow")
            f.restype, f.argtypes = C.c_int, [vp, i64, C.c_size_t, C.c_uint32, vp, i64, C.c_size_t, sz, C.c_size_t, vp]
            for name in ("derivative", "taylor_expansion_of_coeff", "shift_down"):  # the observation ops: x, the order k, the result
                f = getattr(L, pre + name)
                f.restype, f.argtypes = C.c_int, [vp, i64, C.c_size_t, C.c_size_t, vp, i64, C.c_size_t, sz, C.c_size_t, vp]
            f = getattr(L, pre + "evaluate_all_one")
            f.restype, f.argtypes = C.c_int, [vp, i64, C.c_size_t, vp, i64, sz, C.c_size_t, vp]
        L.gft_series_last_form.restype, L.gft_series_last_form.argtypes = C.c_int, []
        _declared = L
    return _declared


def _placed(t, what):
    if t.device.type != "cuda":
        raise TaylorError(f"{what}: the tensor is on {t.device}; it must be in device memory of the library's GPU")


def _check(torch, t, what, series_axis=True, planes=0, placement=True):
    """Everything that can be refused without the library: type, dtype, placement, the series axis (and, for an interval
    tensor, the leading axis of the two planes).  placement=False leaves the placement to a later _placed (series2 judges
    the shapes first)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float64:
        raise TaylorError(f"{what}: the tensor is {t.dtype}; only torch.float64 is accepted (no implicit conversion)")
    if placement:
        _placed(t, what)
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


def _order_short(what, n, ng, ny, names):
    """corr / compose_adj: the result (``n`` coefficients, default ``ng``) is the short side of a transposed operation"""
    if n is None:
        n = ng
    n = int(n)
    if n < 1:
        raise TaylorError(f"{what}: {names[2]} = {n}; the result needs at least one coefficient")
    if ng > MAX_N:
        raise TaylorError(f"{what}: {names[0]} has {ng} coefficients, which exceeds the limit of {MAX_N} per series of this version")
    if n > ng:
        raise TaylorError(f"{what}: {names[2]} = {n} > {ng}, the coefficients of {names[0]} (the result of a transposed operation is its short side)")
    if ny > ng:
        raise TaylorError(f"{what}: {names[1]} has {ny} coefficients, more than the {ng} of {names[0]}")
    return n


def _i64(seq):
    seq = [int(s) for s in seq]
    return (C.c_int64 * max(len(seq), 1))(*seq)


def _run(what, fn_name, x, second, n, out, second_is_seed, names=("x", "y"), e=None, planes=0, max_n=None, short=False):
    """One call of either family.  planes = 1: the tensors are interval tensors [2, B..., n] (seeds [2, B...]); the leading
    axis travels as the first entry of every stride array, which is where the gfti_series_* entry points expect it.
    short: a transposed operation (corr, compose_adj), whose result is no longer than its first operand; names[2] names it."""
    import torch

    _check(torch, x, f"{what}: {names[0]}", planes=planes)
    if second is not None:
        _check(torch, second, f"{what}: {'seed' if second_is_seed else names[1]}", series_axis=not second_is_seed, planes=planes)
    if out is not None:
        _check(torch, out, f"{what}: out", planes=planes)
    lens = (x.shape[-1],) if second_is_seed or second is None else (x.shape[-1], second.shape[-1])
    n = _order_short(what, n, *lens, names) if short else _order(what, n, *lens, max_n=max_n)
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
    if _tracked("series.mul", (x, y), out):
        return _autograd().Mul.apply(x, y, n)
    return _run("series.mul", "gft_series_mul", x, y, n, out, False)


def div(x, y, n=None, out=None):
    """``r[b] = x[b] / y[b]`` to order ``n`` (default ``max(nx, ny)``): the general division recurrence."""
    if _tracked("series.div", (x, y), out):
        return _autograd().Div.apply(x, y, n)
    return _run("series.div", "gft_series_div", x, y, n, out, False)


def exp(x, n=None, seed=None, out=None):
    """``exp(x[b])`` to order ``n`` (default ``nx``).  ``seed``: ``exp(x[b, 0])`` per item (a tensor of the batch shape); with
    the host libm's values the result carries the reference's bits.  ``None``: formed on the device (a few ulps from libm)."""
    if _tracked("series.exp", (x,), out, seed):
        return _autograd().Exp.apply(x, n, seed)
    return _run("series.exp", "gft_series_exp", x, seed, n, out, True)


def log(x, n=None, seed=None, out=None):
    """``log(x[b])`` to order ``n`` (default ``nx``).  ``seed``: ``ln(x[b, 0])`` per item; ``None``: formed on the device (only
    coefficient 0 depends on it)."""
    if _tracked("series.log", (x,), out, seed):
        return _autograd().Log.apply(x, n, seed)
    return _run("series.log", "gft_series_log", x, seed, n, out, True)


def compose(f, g, n=None, out=None):
    """``f[b](g[b])`` truncated at order ``n`` (default ``max(nf, ng)``): Horner over the coefficients of ``f`` with the general
    product at every step, ``res = res * g + f[i]`` for ``i = nf-2 .. 0`` from ``res = [0.0 + f[nf-1]]`` — ``subst_var``'s general
    path without its zero / linear shortcuts, the row resident in LDS across the steps.  About ``nf * n**2 / 2`` multiply-adds per
    item, on one workgroup at most."""
    if _tracked("series.compose", (f, g), out):
        return _autograd().Compose.apply(f, g, n)
    return _run("series.compose", "gft_series_compose", f, g, n, out, False, names=("f", "g"))


def corr(g, y, m=None, out=None):
    """The transposed product, the adjoint of ``mul``: ``<mul(x, y), g> = <x, corr(g, y)>``.  ``g`` has ``ng`` coefficients, ``y``
    has ``ny <= ng``, the result ``m <= ng`` (default ``ng``)::

        c[b, i] = 0.0 + sum_k g[b, k] * y[b, k - i],   k descending from min(ng - 1, i + ny - 1) to i

    multiply and add rounded separately, only stored coefficients entering a sum: bit for bit ``mul(flip(g), y)`` at index
    ``ng - 1 - i``.  ``out`` may be ``g`` itself, never ``y``.  Not differentiable itself (the backward passes are built from it)."""
    return _run("series.corr", "gft_series_corr", g, y, m, out, False, names=("g", "y", "m"), short=True)


def _compose_adj(gh, g, nf, out=None):
    """The transposed Horner loop: the gradient of ``compose(f, g, n)`` with respect to ``f`` (``nf`` coefficients) from the
    gradient ``gh`` of the composition (``n`` coefficients) -- ``a = gh[:l_0]; out[0] = a[0];`` then ``a = corr(a, g, l_{i+1});
    out[i + 1] = a[0]`` at the compact lengths ``l_i = min(1 + (nf - 1 - i)(ng - 1), n)``, in one launch."""
    return _run("series._compose_adj", "gft_series_compose_adj", gh, g, nf, out, False, names=("gh", "g", "nf"), short=True)


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
    e = _exponent("series.pow", e)
    if _tracked("series.pow", (x,), out):
        return _autograd().Pow.apply(x, e, n)
    return _run("series.pow", "gft_series_pow", x, None, n, out, True, e=e)


# ---- the observation ops: derivative, taylor_expansion_of_coeff, shift_down, evaluate_all_one --------------------------------
# One operand, an order k on one axis; the result is k shorter there (include/gftaylor.h states the loops).  _observe serves both
# ranks and both element types: series2, interval_series and interval_series2 call it with their own names and limits.


def _order_k(what, k, length, axis=""):
    """The order of an observation op: an integer with 0 <= k < the stored length on the axis it acts on."""
    import operator

    if isinstance(k, bool):
        raise TypeError(f"{what}: k must be a non-negative integer, got a bool")
    try:
        ki = operator.index(k)
    except TypeError:
        raise TypeError(f"{what}: k must be a non-negative integer, got {k!r}") from None
    if not 0 <= ki < length:
        raise TaylorError(f"{what}: k = {ki}, but x has {length} stored coefficients{axis} (the order must satisfy 0 <= k < {length})")
    return ki


def _observe(what, name, x, k, out, rank=1, var=None, planes=0, limit=None, raw=False):
    """One call of gft[i]_series[2]_<name>.  k is None: evaluate_all_one (the result has the batch shape).  raw: the module has no
    autograd and refuses an operand that requires grad.  Everything that needs no device is judged first."""
    import torch

    ev = k is None
    if rank == 2:
        from . import series2 as mod

        def axes(t, w):
            _check(torch, t, w, series_axis=False, planes=planes, placement=False)
            mod._axes(t, w, planes)
    else:
        mod = None

        def axes(t, w):
            _check(torch, t, w, planes=planes, placement=False)

    axes(x, f"{what}: x")
    if out is not None:
        if ev:
            _check(torch, out, f"{what}: out", series_axis=False, planes=planes, placement=False)
        else:
            axes(out, f"{what}: out")
    shape = tuple(x.shape[-rank:])
    count = shape[0] * shape[-1] if rank == 2 else shape[0]
    if limit is None:
        limit = MAX_N
    if count > limit:
        if rank == 2:
            raise TaylorError(f"{what}: x has {shape[0]} * {shape[1]} = {count} coefficients, which exceeds the limit of {limit} per item of this version")
        raise TaylorError(f"{what}: x has {count} coefficients, which exceeds the limit of {limit} per series of this version")
    axis = -1
    if rank == 2 and not ev:
        if isinstance(var, bool) or not isinstance(var, int) or var not in (0, 1):
            raise TaylorError(f"{what}: var = {var!r}; the variable the operation acts on is 0 (axis -2) or 1 (axis -1)")
        axis = var - 2
    if ev:
        rshape = ()
    else:
        k = _order_k(what, k, shape[axis], f" on axis {axis}" if rank == 2 else "")
        rshape = list(shape)
        rshape[axis] -= k
        rshape = tuple(rshape)
    lead = (2,) * planes
    xbatch = tuple(x.shape[planes:-rank])
    if out is not None:
        nr = len(rshape)
        if out.dim() < planes + nr or tuple(out.shape[out.dim() - nr:]) != rshape:
            raise TaylorError(f"{what}: out has shape {tuple(out.shape)}; the result has {rshape if nr else 'no'} coefficients per item"
                              + (f" (x's {shape}, less k = {k} on the axis)" if nr else " (the batch shape alone)"))
        batch = tuple(out.shape[planes:out.dim() - nr])
        try:
            fits = tuple(torch.broadcast_shapes(xbatch, batch)) == batch
        except RuntimeError:
            fits = False
        if not fits:
            raise TaylorError(f"{what}: out has batch shape {batch}; the operand has {xbatch}")
    else:
        batch = xbatch
    if raw and torch.is_grad_enabled() and x.requires_grad:
        raise TaylorError(f"{what}: an operand requires grad, and this version of {what.split('.')[0]} has no autograd; pass x.detach() or call "
                          "under torch.no_grad() (nothing is detached silently)")
    _placed(x, f"{what}: x")
    if out is not None:
        _placed(out, f"{what}: out")
        if out.device != x.device:
            raise TaylorError(f"{what}: the tensors are on different devices ({x.device}, {out.device})")
    else:
        out = torch.empty(lead + batch + rshape, dtype=torch.float64, device=x.device)
    nb = len(batch)
    if planes and x.dim() < nb + 1 + rank:  # the plane axis stays first, missing batch axes go behind it (a view)
        x = x[(slice(None),) + (None,) * (nb + 1 + rank - x.dim())]
    L = mod._lib() if mod else _lib()
    dev = int(L.gft_device())
    if dev >= 0 and x.device.index != dev:
        raise TaylorError(f"{what}: the tensors are on {x.device}, but the library runs on cuda:{dev}")
    ns = nb + planes
    xe = x.expand(lead + batch + shape)
    bsz = (C.c_size_t * max(nb, 1))(*batch)
    stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    fn = getattr(L, ("gfti_" if planes else "gft_") + ("series2_" if rank == 2 else "series_") + name)
    xa = (C.c_void_p(xe.data_ptr()), _i64(xe.stride()[:ns])) + ((xe.stride(-2),) if rank == 2 else ()) + shape
    ra = (C.c_void_p(out.data_ptr()), _i64(out.stride()[:ns]))
    if ev:
        rc = fn(*xa, *ra, bsz, nb, stream)
    else:
        ka = (C.c_int(var), k) if rank == 2 else (k,)
        rc = fn(*xa, *ka, *ra, *((out.stride(-2),) if rank == 2 else ()), *rshape, bsz, nb, stream)
    if rc != 0:
        raise TaylorError((L.gft_last_error() or b"unknown error").decode())
    return out


def derivative(x, k, out=None):
    """The ``k``-th derivative's coefficients: ``out[b, j] = x[b, k + j] * ff_j`` for ``j < nx - k``, one rounding each, with the
    reference's running-product factors ``ff_0 = k!``, ``ff_{j+1} = ff_j * ((k + j + 1) / (j + 1))`` (the quotient rounded first)."""
    if _tracked("series.derivative", (x,), out):
        return _autograd().observe("series", 1).Derivative.apply(x, None, k)
    return _observe("series.derivative", "derivative", x, k, out)


def taylor_expansion_of_coeff(x, k, out=None):
    """The expansion of coefficient ``k``: ``out[b, 0] = x[b, k]`` and ``out[b, j] = x[b, k + j] * f_j`` with ``f_0 = 1``,
    ``f_j = f_{j-1} * ((k + j) / j)`` -- ``derivative`` without its factor ``k!``."""
    if _tracked("series.taylor_expansion_of_coeff", (x,), out):
        return _autograd().observe("series", 1).Coeff.apply(x, None, k)
    return _observe("series.taylor_expansion_of_coeff", "taylor_expansion_of_coeff", x, k, out)


def shift_down(x, k, out=None):
    """The coefficients moved down by ``k``, those pushed out gathered at 0: ``out[b, 0] = x[b, k] + (0.0 + x[b, 0] + ... +
    x[b, k - 1])`` (ascending; with ``nx == k + 1`` the ascending sum of all of them) and ``out[b, j] = x[b, k + j]``."""
    if _tracked("series.shift_down", (x,), out):
        return _autograd().observe("series", 1).ShiftDown.apply(x, None, k)
    return _observe("series.shift_down", "shift_down", x, k, out)


def evaluate_all_one(x, out=None):
    """The series at ``t = 1``: ``0.0 + x[b, 0] + x[b, 1] + ...``, one ascending chain per item; the result has the batch shape."""
    if _tracked("series.evaluate_all_one", (x,), out):
        return _autograd().observe("series", 1).EvalOne.apply(x)
    return _observe("series.evaluate_all_one", "evaluate_all_one", x, None, out)


# ---- autograd ----------------------------------------------------------------------------------------------------------------
# Every vector-Jacobian product below is a sequence of this module's own calls on detached tensors; `corr` carries the order of
# its sums, so a gradient's bits are pinned up to the reduction over broadcast batch axes (sum_to_size: torch's order).


def _tracked(what, operands, out, seed=None):
    """Whether the call records a grad_fn: grad mode is on and an operand requires grad.  Refuses what cannot be differentiated."""
    try:
        import torch
    except ImportError:  # the type check of _run reports it
        return False
    if not torch.is_grad_enabled():
        return False
    if isinstance(seed, torch.Tensor) and seed.requires_grad:
        raise TaylorError(f"{what}: seed requires grad; the seed is exp(x[..., 0]) / ln(x[..., 0]) by contract and the gradient flows to x "
                          "(pass seed.detach())")
    if not any(isinstance(t, torch.Tensor) and t.requires_grad for t in operands):
        return False
    if out is not None:
        raise TaylorError(f"{what}: out= cannot be combined with an operand that requires grad (the functions with out= do not support "
                          "automatic differentiation)")
    return True


_functions = None


def _autograd():
    """The torch.autograd.Function of every operation (built on first use: this module imports without torch)."""
    global _functions
    if _functions is not None:
        return _functions
    import types

    import torch
    from torch.autograd.function import once_differentiable

    def unit_stride(g):  # z.sum().backward() hands over an expanded scalar: stride 0 on the series axis
        return g if g.shape[-1] == 1 or g.stride(-1) == 1 else g.contiguous()

    def one(t):
        return torch.ones(1, dtype=torch.float64, device=t.device)

    class Mul(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y, n):
            x, y = x.detach(), y.detach()
            ctx.save_for_backward(x, y)
            return _run("series.mul", "gft_series_mul", x, y, n, None, False)

        @staticmethod
        @once_differentiable
        def backward(ctx, gz):
            x, y = ctx.saved_tensors
            gz = unit_stride(gz)
            gx = corr(gz, y, x.shape[-1]).sum_to_size(x.shape) if ctx.needs_input_grad[0] else None
            gy = corr(gz, x, y.shape[-1]).sum_to_size(y.shape) if ctx.needs_input_grad[1] else None
            return gx, gy, None

    class Div(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y, n):
            x, y = x.detach(), y.detach()
            r = _run("series.div", "gft_series_div", x, y, n, None, False)
            ctx.save_for_backward(r, y)
            ctx.shapes = (x.shape, y.shape)
            return r

        @staticmethod
        @once_differentiable
        def backward(ctx, gr):
            r, y = ctx.saved_tensors
            xs, ys = ctx.shapes
            n = r.shape[-1]
            u = corr(unit_stride(gr), div(one(y), y, n), n)  # the gradient of the dividend at full length
            gx = u[..., :xs[-1]].sum_to_size(xs) if ctx.needs_input_grad[0] else None
            gy = (-corr(u, r, ys[-1])).sum_to_size(ys) if ctx.needs_input_grad[1] else None
            return gx, gy, None

    class Exp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, n, seed):
            x = x.detach()
            e = _run("series.exp", "gft_series_exp", x, seed, n, None, True)
            ctx.save_for_backward(e)
            ctx.shape = x.shape
            return e

        @staticmethod
        @once_differentiable
        def backward(ctx, ge):
            (e,) = ctx.saved_tensors
            return corr(unit_stride(ge), e, ctx.shape[-1]).sum_to_size(ctx.shape), None, None

    class Log(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, n, seed):
            x = x.detach()
            ctx.save_for_backward(x)
            return _run("series.log", "gft_series_log", x, seed, n, None, True)

        @staticmethod
        @once_differentiable
        def backward(ctx, gl):
            (x,) = ctx.saved_tensors
            n = gl.shape[-1]
            return corr(unit_stride(gl), div(one(x), x, n), x.shape[-1]).sum_to_size(x.shape), None, None

    class Pow(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, e, n):
            x = x.detach()
            ctx.save_for_backward(x)
            ctx.e = e
            return _run("series.pow", "gft_series_pow", x, None, n, None, True, e=e)

        @staticmethod
        @once_differentiable
        def backward(ctx, gp):
            (x,) = ctx.saved_tensors
            if ctx.e == 0:
                return torch.zeros_like(x), None, None
            n = gp.shape[-1]
            return (ctx.e * corr(unit_stride(gp), pow(x, ctx.e - 1, n), x.shape[-1])).sum_to_size(x.shape), None, None

    class Compose(torch.autograd.Function):
        @staticmethod
        def forward(ctx, f, g, n):
            f, g = f.detach(), g.detach()
            ctx.save_for_backward(f, g)
            return _run("series.compose", "gft_series_compose", f, g, n, None, False, names=("f", "g"))

        @staticmethod
        @once_differentiable
        def backward(ctx, gh):
            f, g = ctx.saved_tensors
            gh = unit_stride(gh)
            n, nf = gh.shape[-1], f.shape[-1]
            gf = gg = None
            if ctx.needs_input_grad[0]:
                gf = _compose_adj(gh, g, nf).sum_to_size(f.shape)
            if ctx.needs_input_grad[1]:  # h = f(g): dh = f'(g) * dg
                if nf > 1:
                    fp = f[..., 1:] * torch.arange(1, nf, dtype=torch.float64, device=f.device)
                else:
                    fp = torch.zeros_like(f)
                gg = corr(gh, compose(fp, g, n), g.shape[-1]).sum_to_size(g.shape)
            return gf, gg, None

    # The observation ops are linear maps; their adjoints are torch indexing around this module's own calls.  One set of
    # Functions per (module, rank): series at rank 1, series2_grad at rank 2 (var is None at rank 1).
    observers = {}

    def observe(module, rank):
        if (module, rank) in observers:
            return observers[(module, rank)]

        def axis_of(var):
            return -1 if rank == 1 else var - 2

        def scaled(name, long_name):
            class Scaled(torch.autograd.Function):
                @staticmethod
                def forward(ctx, x, var, k):
                    x = x.detach()
                    ctx.var, ctx.shape = var, x.shape
                    z = _observe(f"{module}.{long_name}", long_name, x, k, None, rank=rank, var=var)
                    ctx.k = x.shape[axis_of(var)] - z.shape[axis_of(var)]
                    return z

                @staticmethod
                @once_differentiable
                def backward(ctx, gz):  # gx[k + j] = gz[j] * factor_j, the factors the forward op of ones; gx[< k] = +0.0
                    ax, k = axis_of(ctx.var), ctx.k
                    ln = ctx.shape[ax]
                    fac = _observe(f"{module}.{long_name}", long_name, torch.ones(ln, dtype=torch.float64, device=gz.device), k, None)
                    gx = torch.zeros(ctx.shape, dtype=torch.float64, device=gz.device)
                    gx.narrow(ax, k, ln - k).copy_(gz * (fac if ax == -1 else fac[:, None]))
                    return gx, None, None

            Scaled.__name__ = Scaled.__qualname__ = name
            return Scaled

        class ShiftDown(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, var, k):
                x = x.detach()
                ctx.var = var
                z = _observe(f"{module}.shift_down", "shift_down", x, k, None, rank=rank, var=var)
                ctx.k = x.shape[axis_of(var)] - z.shape[axis_of(var)]
                return z

            @staticmethod
            @once_differentiable
            def backward(ctx, gz):  # gx[i] = gz[0] for i <= k, gx[k + j] = gz[j] for j >= 1
                ax, k = axis_of(ctx.var), ctx.k
                if k == 0:
                    return gz, None, None
                head = gz.narrow(ax, 0, 1)
                return torch.cat([head.expand(*(k if a == gz.dim() + ax else s for a, s in enumerate(gz.shape))), gz], dim=ax), None, None

        class EvalOne(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x):
                x = x.detach()
                ctx.shape = x.shape
                return _observe(f"{module}.evaluate_all_one", "evaluate_all_one", x, None, None, rank=rank)

            @staticmethod
            @once_differentiable
            def backward(ctx, gz):  # gz broadcast over the item
                return gz[(...,) + (None,) * rank].expand(ctx.shape)

        ns = types.SimpleNamespace(Derivative=scaled("Derivative", "derivative"), Coeff=scaled("Coeff", "taylor_expansion_of_coeff"),
                                   ShiftDown=ShiftDown, EvalOne=EvalOne)
        observers[(module, rank)] = ns
        return ns

    _functions = types.SimpleNamespace(Mul=Mul, Div=Div, Exp=Exp, Log=Log, Pow=Pow, Compose=Compose, observe=observe)
    return _functions


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
