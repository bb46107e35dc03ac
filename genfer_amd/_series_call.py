"""The one host path of the batched series modules: ``series``, ``series2``, ``series3``, ``interval_series``, ``interval_series2``,
``interval_series3`` (and the
autograd Functions of ``series`` and ``series2_grad``) describe a call by data and hand it to ``run``.

``OPS`` (and ``MORE_OPS``, the operations added behind it) is the table of the operations: one row says what travels between the first operand and the result, which side is the long
one, the operands' names in messages and whether ``var`` travels at ranks 2 and 3.  The same rows build the ctypes declarations of every
``gft[i]_series[2]_*`` and ``gftb_series_*`` entry point and the argument tuple of a call (``_arguments``), so the two cannot drift apart; the C layer's
counterpart is ``gft::SERIES_OPS`` (gft_series_args.hpp), and tests/test_series_refusals.py holds the two tables together.  A ``Call``
says the rest: the rank (1: the last axis is the series, 2 / 3: the last two / three axes are the coefficient array), ``planes`` (1: interval
tensors ``[2, B..., item]``, the plane axis travelling as the first entry of every batch-stride array), the limit of the long side
and the module's name for messages, and ``elem``, what the planes hold (``ELEMS``: the symbol prefix and the words of the messages; ``"bigfloat"``
is ``bigfloat_series``, rank 1's six arithmetic ops).  ``run`` works on ``t.shape[-rank:]`` and ``t.stride()[-rank:-1]``: rank 2 contributes its row
stride and its second length because those tuples are one entry longer, rank 3 its slab stride and third length likewise.

Everything that needs no device is judged first, in one order for every module: type, dtype, planes, axes (per tensor), the orders,
``out``, grad, then the placement, the devices and the library's device.  ``run``, ``run_chain`` (``observe_chain``, whose items
carry their own scalars ``x``, ``cs``) and ``run_linear`` (``mul_linear`` and ``compose_linear``: ``c``, ``m``) hold the shape rules
of their operations and end in the one tail ``_launch``; ``_axes`` is the one check of the series axes, by the rank.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

from .taylor import TaylorError

# kind: "second" (a second series), "seed" (exp / log: one value per item, or None), "e" (pow's exponent), "k" (the order of an
# observation op) or None (evaluate_all_one: the result has the batch shape).  long: the side that carries the limit and bounds the
# others -- the result, or x for the transposed and the observation ops.  names: the operands (and, transposed, the result's
# order) in messages.  var: the variable travels at ranks 2 and 3, behind the operands.  label: the function's name in messages.
Op = namedtuple("Op", "suffix kind long names var label")
# raw: the module has no autograd and refuses an operand that requires grad.  elem: what the planes hold, a key of ELEMS (None: by the
# planes alone -- float64 or Interval<F64>)
Call = namedtuple("Call", "module rank planes limit raw elem", defaults=(None,))
# per element kind: the symbol prefix, what a tensor is called and what its two planes are, and whether a plane stride of 0 is a value
# (a point interval) or a mistake (a factor plane is not its own exponent plane)
Elem = namedtuple("Elem", "prefix noun planes point")
ELEMS = {"interval": Elem("gfti_", "an interval tensor", "(lo, hi)", True),
         "bigfloat": Elem("gftb_", "a BigFloat tensor", "(factor, exponent)", False)}
BIGFLOAT_OPS = ("mul", "div", "exp", "log", "compose", "pow")  # gftb_series_*: rank 1 only


def _elem(call):
    """the Elem of a call with planes (None: one plane, float64)"""
    return ELEMS[call.elem or "interval"] if call.planes else None


def _op(suffix, kind, long="result", names=("x", "y"), var=False, label=None):
    return Op(suffix, kind, long, names, var, label or suffix)


OPS = {o.suffix: o for o in (
    _op("mul", "second"),
    _op("div", "second"),
    _op("exp", "seed"),
    _op("log", "seed"),
    _op("compose", "second", names=("f", "g"), var=True),
    _op("pow", "e"),
    _op("corr", "second", long="x", names=("g", "y", "m")),
    _op("compose_adj", "second", long="x", names=("gh", "g", "nf"), var=True, label="_compose_adj"),
    _op("derivative", "k", long="x", var=True),
    _op("taylor_expansion_of_coeff", "k", long="x", var=True),
    _op("shift_down", "k", long="x", var=True),
    _op("evaluate_all_one", None, long="x"),
    # kind "chain": the operand a, at rank 2 the axis, then the scalars x and the constants cs of every item (a pointer and batch
    # strides each, as the seeds), nsteps and degree_p1 (run_chain)
    _op("observe_chain", "chain", long="x", names=("a", "x", "cs"), var=True),
    # kind "linear": the operand, at rank 2 its `var` axes (mul_linear: the factor's variable; compose_linear: var and wvar), then the
    # scalars c and m of every item (a pointer and batch strides each, as the seeds) (run_linear)
    _op("mul_linear", "linear", names=("a", "c", "m"), var=1),
    _op("compose_linear", "linear", names=("f", "c", "m"), var=2),
)}
# The operations behind the table (gft::SERIES_MORE_OPS): OPS ends with the affine substitutions -- tests/test_series_linear_cpu.py pins
# them as its last rows, and tests/test_series_refusals.py holds OPS to gft::SERIES_OPS row by row -- so later operations are stated here.
MORE_OPS = {o.suffix: o for o in (
    # kind "negbin": the chain's layout with the scalars p behind x (a pointer and batch strides), the row ls where the chain has cs,
    # and the two counts nls = order + 1 and degree_p1 (run_negbinomial)
    _op("observe_negbinomial", "negbin", long="x", names=("a", "x", "ls"), var=True),
    # kind "lah": the scalars p (a pointer and batch strides), the order, the result (run_lah_row).  One entry point per element
    # type, gft[i]_series_lah_row: the operand has no series axis, so there is no series2_ spelling
    _op("lah_row", "lah", names=("p", None)),
)}
F64_ONLY = ("corr", "compose_adj")  # no gfti_ twin
RANK3 = ("mul", "div", "exp", "log", "compose", "pow")  # gft[i]_series3_*: the core operations, compose and pow


def _i64(seq):
    seq = [int(s) for s in seq]
    return (C.c_int64 * max(len(seq), 1))(*seq)


_I64P, _SZP = C.POINTER(C.c_int64), C.POINTER(C.c_size_t)


def _view_types(rank, lens=True):
    """an operand in an entry point's argument list: the pointer, the batch strides, and with ``lens`` the row strides (rank 2
    has one, rank 3 the slab stride in front of it) and the lengths"""
    return (C.c_void_p, _I64P) + ((C.c_int64,) * (rank - 1) + (C.c_size_t,) * rank if lens else ())


def _view(rank, t, ns, lens=True):
    """the values of _view_types for a tensor (None: no seeds); ``ns``: the leading strides that are batch strides"""
    if t is None:
        return (None, None)
    v = (C.c_void_p(t.data_ptr()), _i64(t.stride()[:ns]))
    return v + t.stride()[-rank:-1] + tuple(t.shape[-rank:]) if lens else v


def _arguments(op, rank, view, e, var, k, tail):
    """The argument list of gft[i]_series[2]_<op.suffix>, from the op's row.  ``view(which, lens)`` gives the part of an operand
    ("x", "second", "out"), the others are the parts of the scalars and of the tail (the batch shape, its length, the stream):
    ctypes for the declaration, values for a call -- one layout for both."""
    a = view("x", True)
    if op.kind == "chain":  # (k: the two counts nsteps, degree_p1)
        return a + (var if rank >= 2 else ()) + view("second", False) + view("cs", False) + k + view("out", True) + tail
    if op.kind == "negbin":  # (k: the two counts nls, degree_p1)
        return a + (var if rank >= 2 else ()) + view("second", False) + view("p", False) + view("cs", False) + k + view("out", True) + tail
    if op.kind == "lah":  # (k: the order)
        return view("x", False) + k + view("out", False) + tail
    if op.kind == "linear":  # (var: op.var axes)
        return a + (var if rank >= 2 else ()) + view("second", False) + view("cs", False) + view("out", True) + tail
    if op.kind == "second":
        a += view("second", True)
    elif op.kind == "seed":
        a += view("second", False)
    elif op.kind == "e":
        a += e
    if op.var and rank >= 2:
        a += var
    if op.kind == "k":
        a += k
    return a + view("out", op.kind is not None) + tail


_declared = None


def _lib():
    """The library with every batched series entry point declared from OPS."""
    global _declared
    if _declared is None:
        from . import lib

        L = lib()
        for pre in ("gft_", "gfti_"):  # the interval twins take the same argument lists
            for rank, mid in ((1, "series_"), (2, "series2_")):
                for op in list(OPS.values()) + list(MORE_OPS.values()):
                    if op.kind == "lah" and rank == 2:
                        continue
                    if pre == "gft_" or op.suffix not in F64_ONLY:
                        f = getattr(L, pre + mid + op.suffix)
                        f.restype = C.c_int
                        f.argtypes = list(_arguments(op, rank, lambda which, lens: _view_types(rank, lens), (C.c_uint32,), (C.c_int,) * int(op.var),
                                                     (C.c_size_t,) * (2 if op.kind in ("chain", "negbin") else 1), (_SZP, C.c_size_t, C.c_void_p)))
        for suffix in BIGFLOAT_OPS:  # the BigFloat family: gfti_series_*'s argument lists, from the same rows
            f = getattr(L, ELEMS["bigfloat"].prefix + "series_" + suffix)
            f.restype = C.c_int
            f.argtypes = list(_arguments(OPS[suffix], 1, lambda which, lens: _view_types(1, lens), (C.c_uint32,), (), (C.c_size_t,),
                                         (_SZP, C.c_size_t, C.c_void_p)))
        for pre in ("gft_", "gfti_"):
            for suffix in RANK3:
                f = getattr(L, pre + "series3_" + suffix)
                f.restype = C.c_int
                f.argtypes = list(_arguments(OPS[suffix], 3, lambda which, lens: _view_types(3, lens), (C.c_uint32,), (C.c_int,), (),
                                             (_SZP, C.c_size_t, C.c_void_p)))
        L.gft_series_last_form.restype, L.gft_series_last_form.argtypes = C.c_int, []
        _declared = L
    return _declared


def _placed(t, what):
    if t.device.type != "cuda":
        raise TaylorError(f"{what}: the tensor is on {t.device}; it must be in device memory of the library's GPU")


def _check(torch, t, what, planes=0, elem=None):
    """type, dtype and, for a tensor of two planes (``elem``: its Elem), the leading axis of the planes and its stride"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float64:
        raise TaylorError(f"{what}: the tensor is {t.dtype}; only torch.float64 is accepted (no implicit conversion)")
    if planes and (t.dim() < 1 or t.shape[0] != 2):
        lead = "no axes" if t.dim() < 1 else f"a first axis of {t.shape[0]}"
        elem = elem or ELEMS["interval"]
        raise TaylorError(f"{what}: the tensor has {lead}; {elem.noun} is stacked [2, ...] = {elem.planes} along its first axis")
    if planes and elem is not None and not elem.point and t.stride(0) == 0:
        raise TaylorError(f"{what}: the tensor has plane stride 0 (an expanded first axis); the two planes of {elem.noun} are {elem.planes}, "
                          "and a factor plane cannot be its own exponent plane")


def _axes(rank, t, what, planes=0):
    """the ``rank`` series axes of an operand or of ``out``: enough axes, none empty, the last one with unit stride"""
    kind, count = (None, "bivariate", "trivariate")[rank - 1], (None, "two", "three")[rank - 1]
    if t.dim() < rank + planes:
        if rank == 1:
            raise TaylorError(f"{what}: a 0-dimensional tensor has no series axis")
        if planes:
            raise TaylorError(f"{what}: the tensor has {t.dim()} axes; a {kind} interval series needs at least {rank + 1} (the first holds the two "
                              f"planes, the last {count} are the coefficient array)")
        raise TaylorError(f"{what}: the tensor has {t.dim()} axes; a {kind} series needs at least {rank} (the last {count} are the coefficient array)")
    if 0 in t.shape[-rank:]:
        raise TaylorError(f"{what}: the series (last) axis is empty" if rank == 1 else
                          f"{what}: a series axis is empty (the last {count} axes are {tuple(t.shape[-rank:])})")
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        raise TaylorError(f"{what}: the series (last) axis has stride {t.stride(-1)}; it must have unit stride")


_rank = {}


def _rank_rules(rank):
    """What differs by rank beyond _axes: the order helpers (they stay with their modules, series._order ... and
    series2._orders ...; here they take and give item shapes) and the texts that count "per series" or "per item"."""
    if not _rank:
        from .series import _order, _order_short
        from .series2 import _orders, _orders_short
        from .series3 import _orders as _orders3

        _rank[1] = (lambda what, n, limit, *items: (_order(what, n, *[i[0] for i in items], max_n=limit),),
                    lambda what, n, names, g, y: (_order_short(what, n, g[0], y[0], names),),
                    "{what}: x has {count} coefficients, which exceeds the limit of {limit} per series of this version",
                    "{what}: out has {got[0]} coefficients per series, the result has n = {want[0]}")
        _rank[2] = (lambda what, n, limit, *items: _orders(what, n, *items, max_elems=limit),
                    lambda what, n, names, g, y: _orders_short(what, n, g, y, names),
                    "{what}: x has {shape[0]} * {shape[1]} = {count} coefficients, which exceeds the limit of {limit} per item of this version",
                    "{what}: out has {got} coefficients per item, the result has n = {want}")
        _rank[3] = (lambda what, n, limit, *items: _orders3(what, n, *items, max_elems=limit), None, None,
                    "{what}: out has {got} coefficients per item, the result has n = {want}")  # (no transposed or observation op at rank 3)
    return _rank[rank]


def _launch(what, op, call, named, out, batch, rshape, scalars):
    """The tail of every call, once.  ``named``: the operands as (the part's key for ``_arguments``, the name in messages, the tensor
    or None, the item shape it is expanded to behind the batch), in the order they are judged; ``out`` (None: allocated here) follows
    them.  ``scalars``: the ``e``, ``var`` and ``k`` parts of the argument list.  In this order: the placement of every tensor, one
    device, ``out``, the interval operands lifted to the batch's axes, the library's device, the expansion, the call, its error."""
    import torch

    _module, rank, planes, _limit, _raw, _kind = call
    given = [(t, name) for _, name, t, _ in named if t is not None] + ([(out, "out")] if out is not None else [])
    for t, name in given:
        _placed(t, f"{what}: {name}")
    device = given[0][0].device
    for t, _ in given[1:]:
        if t.device != device:
            raise TaylorError(f"{what}: the tensors are on different devices ({device}, {t.device})")
    lead, nb = (2,) * planes, len(batch)
    if out is None:
        out = torch.empty(lead + batch + rshape, dtype=torch.float64, device=device)
    parts = {key: t for key, _, t, _ in named}
    if planes:  # torch aligns shapes from the right: the plane axis stays first, missing batch axes go behind it (a view)
        for key, _, t, item in named:
            if t is not None and t.dim() < nb + 1 + len(item):
                parts[key] = t[(slice(None),) + (None,) * (nb + 1 + len(item) - t.dim())]
    L = _lib()
    dev = int(L.gft_device())
    if dev >= 0 and device.index != dev:
        raise TaylorError(f"{what}: the tensors are on {device}, but the library runs on cuda:{dev}")
    for key, _, t, item in named:
        if t is not None:
            parts[key] = parts[key].expand(lead + batch + item)
    parts["out"] = out
    ns = nb + planes  # entries of a batch-stride array
    tail = ((C.c_size_t * max(nb, 1))(*batch), nb, C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    fn = getattr(L, (_elem(call).prefix if planes else "gft_") + ("series_", "series2_", "series3_")[rank - 1] + op.suffix)
    if fn(*_arguments(op, rank, lambda which, lens: _view(rank, parts[which], ns, lens), *scalars, tail)) != 0:
        raise TaylorError((L.gft_last_error() or b"unknown error").decode())
    return out


def run(call, name, x, second=None, n=None, out=None, scalar=None, var=None):
    """One call of gft[i]_series[2]_<name>.  ``second``: the second series or the seeds; ``scalar``: pow's ``e`` or an observation
    op's ``k``; ``var``: the variable at ranks 2 and 3 (already judged by series2._var / series3._var where it is compose's)."""
    import torch

    op, (module, rank, planes, limit, raw, _kind) = OPS[name], call
    what = f"{module}.{op.label}"
    elem = _elem(call)
    order, short, over_text, out_text = _rank_rules(rank)
    observe, seeded = op.kind in ("k", None), op.kind == "seed"
    xname, sname = op.names[0], "seed" if seeded else op.names[1]
    # everything that needs no device first: types, shapes, strides, orders, out, grad -- then the placement
    for t, w, item in ((x, xname, True), (second, sname, not seeded), (out, "out", op.kind is not None)):
        if t is not None:
            w = f"{what}: {w}"
            _check(torch, t, w, planes, elem)
            if item:
                _axes(rank, t, w, planes)
    shape = tuple(x.shape[-rank:])
    if observe:
        count = shape[0] * shape[-1] if rank == 2 else shape[0]
        if count > limit:
            raise TaylorError(over_text.format(what=what, shape=shape, count=count, limit=limit))
        axis = -1
        if op.var and rank == 2:
            from .series2 import _var

            axis = _var(what, var, "the variable the operation acts on is 0 (axis -2) or 1 (axis -1)") - 2
        rshape = ()
        if op.kind == "k":
            from .series import _order_k

            scalar = _order_k(what, scalar, shape[axis], f" on axis {axis}" if rank == 2 else "")
            rshape = shape[:axis] + (shape[axis] - scalar,) + shape[rank + axis + 1:]
    elif op.long == "x":
        rshape = short(what, n, op.names, shape, tuple(second.shape[-rank:]))
    else:
        rshape = order(what, n, limit, shape, *((tuple(second.shape[-rank:]),) if op.kind == "second" else ()))
    nr = len(rshape)
    shapes = [x.shape[planes:-rank]]
    if second is not None:
        shapes.append(second.shape[planes:] if seeded else second.shape[planes:-rank])
    same = all(s == shapes[0] for s in shapes)  # (the common case, without torch.broadcast_shapes)
    if out is None:
        batch = tuple(shapes[0] if same else torch.broadcast_shapes(*shapes))
    else:
        if out.dim() < planes + nr or tuple(out.shape[out.dim() - nr:]) != rshape:
            if observe:
                raise TaylorError(f"{what}: out has shape {tuple(out.shape)}; the result has {rshape if nr else 'no'} coefficients per item"
                                  + (f" (x's {shape}, less k = {scalar} on the axis)" if nr else " (the batch shape alone)"))
            raise TaylorError(out_text.format(what=what, got=tuple(out.shape[-rank:]), want=rshape))
        batch = tuple(out.shape[planes:out.dim() - nr])
        try:
            fits = same and shapes[0] == batch or tuple(torch.broadcast_shapes(*shapes, batch)) == batch
        except RuntimeError:
            if not observe:  # (torch's own message for operands that do not broadcast against out)
                raise
            fits = False
        if not fits:
            if observe:
                raise TaylorError(f"{what}: out has batch shape {batch}; the operand has {tuple(shapes[0])}")
            raise TaylorError(f"{what}: out has batch shape {batch}; the operands broadcast to {tuple(torch.broadcast_shapes(*shapes))}")
    if raw and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, second)):
        raise TaylorError(f"{what}: an operand requires grad, and this version of {module} has no autograd; pass {xname}.detach() or call under "
                          "torch.no_grad() (nothing is detached silently)")
    named = (("x", xname, x, shape), ("second", sname, second, () if seeded or second is None else tuple(second.shape[-rank:])))
    return _launch(what, op, call, named, out, batch, rshape, ((scalar,), (var,), (scalar,)))


def _count(what, name, v):
    """one of the chain's counts: an integer, no bool"""
    import operator

    if isinstance(v, bool):
        raise TypeError(f"{what}: {name} must be an integer, got a bool")
    try:
        return operator.index(v)
    except TypeError:
        raise TypeError(f"{what}: {name} must be an integer, got {v!r}") from None


def run_chain(call, a, var, x, cs, degree_p1=None, out=None):
    """One call of gft[i]_series[2]_observe_chain: ``a`` the operand, ``var`` the axis at rank 2, ``x`` one scalar per item or None
    (the continuous form), ``cs`` the constants ``[B..., nsteps]``.  The checks come in ``run``'s order."""
    import torch

    op, (module, rank, planes, limit, _raw, _kind) = OPS["observe_chain"], call
    what = f"{module}.{op.label}"
    over_text = _rank_rules(rank)[2]
    for t, w in ((a, "a"), (x, "x"), (cs, "cs"), (out, "out")):
        if t is None and w in ("x", "out"):
            continue
        w = f"{what}: {w}"
        _check(torch, t, w, planes)
        if t is a or t is out:
            _axes(rank, t, w, planes)
    if cs.dim() < 1 + planes:
        raise TaylorError(f"{what}: cs has no axis of constants; it is [{'2, ' if planes else ''}B..., nsteps]")
    if cs.shape[-1] > 1 and cs.stride(-1) != 1:
        raise TaylorError(f"{what}: cs: the last axis (the steps) has stride {cs.stride(-1)}; it must have unit stride")
    shape = tuple(a.shape[-rank:])
    count = shape[0] * shape[-1] if rank == 2 else shape[0]
    if count > limit:
        raise TaylorError(over_text.format(what=what, shape=shape, count=count, limit=limit).replace(": x has", ": a has"))
    axis = -1
    if rank == 2:
        from .series2 import _var

        axis = _var(what, var, "the variable the chain acts on is 0 (axis -2) or 1 (axis -1)") - 2
    length, nsteps, on = shape[axis], int(cs.shape[-1]), f" on axis {axis}" if rank == 2 else ""
    if nsteps == 0:
        raise TaylorError(f"{what}: nsteps = 0 (cs holds no constants: a chain has at least one step)")
    d = length - nsteps if degree_p1 is None else _count(what, "degree_p1", degree_p1)
    if d < 2:
        raise TaylorError(f"{what}: degree_p1 = {d} (the result needs at least two coefficients{on}: degree_p1 >= 2"
                          + (f"; the default is {length} - nsteps)" if degree_p1 is None else ")"))
    if d + nsteps > length:
        raise TaylorError(f"{what}: degree_p1 + nsteps = {d} + {nsteps}, but a has {length} stored coefficients{on} (every step takes one: "
                          f"degree_p1 + nsteps <= {length})")
    rshape = (d,) if rank == 1 else ((d, min(shape[1], d)) if axis == -2 else (min(shape[0], d), d))
    named = [("a", a.shape[planes:a.dim() - rank])] + ([("x", x.shape[planes:])] if x is not None else []) + [("cs", cs.shape[planes:-1])]
    try:
        batch = tuple(torch.broadcast_shapes(*[s for _, s in named]))
    except RuntimeError:
        raise TaylorError(f"{what}: the batch shapes do not broadcast: " + ", ".join(f"{n} has {tuple(s)}" for n, s in named)
                          + " (x has the batch shape, cs the batch shape and one last axis of nsteps constants)") from None
    if out is not None:
        if out.dim() < planes + rank or tuple(out.shape[-rank:]) != rshape:
            raise TaylorError(f"{what}: out has shape {tuple(out.shape)}; the result has {rshape} coefficients per item (degree_p1 = {d}{on})")
        if tuple(out.shape[planes:out.dim() - rank]) != batch:
            raise TaylorError(f"{what}: out has batch shape {tuple(out.shape[planes:out.dim() - rank])}; the operands broadcast to {batch}")
    if torch.is_grad_enabled():
        for t, w in ((a, "a"), (x, "x"), (cs, "cs")):
            if t is not None and t.requires_grad:
                raise TaylorError(f"{what}: {w} requires grad, and observe_chain has no autograd in this version; pass {w}.detach() or call "
                                  "under torch.no_grad() (nothing is detached silently)")
    named = (("x", "a", a, shape), ("second", "x", x, ()), ("cs", "cs", cs, (nsteps,)))
    return _launch(what, op, call, named, out, batch, rshape, ((), (var,), (nsteps, d)))


def run_linear(call, name, a, var, wvar, c, m, n=None, out=None):
    """One call of gft[i]_series[2]_mul_linear / _compose_linear: ``a`` the operand, ``var`` (and compose_linear's ``wvar``) the axes at
    rank 2, ``c`` and ``m`` one scalar per item each, ``n`` the result's order (an int at rank 1, a pair at rank 2).  The checks come in
    ``run``'s order."""
    import torch

    op, (module, rank, planes, limit, _raw, _kind) = OPS[name], call
    what = f"{module}.{op.label}"
    comp = name == "compose_linear"
    aname = op.names[0]
    for t, w in ((a, aname), (c, "c"), (m, "m"), (out, "out")):
        if t is None and w == "out":
            continue
        w = f"{what}: {w}"
        _check(torch, t, w, planes)
        if t is a or t is out:
            _axes(rank, t, w, planes)
    shape = tuple(a.shape[-rank:])
    v = w = rank - 1  # as positions of an item's shape
    if rank == 2:
        from .series2 import _var

        v = w = _var(what, var, "the variable of f that is replaced is 0 (axis -2) or 1 (axis -1)" if comp
                     else "the variable of the linear factor is 0 (axis -2) or 1 (axis -1)")
        if comp and wvar is not None:
            if isinstance(wvar, bool) or not isinstance(wvar, int) or wvar not in (0, 1):
                raise TaylorError(f"{what}: wvar = {wvar!r}; the variable of the affine series is 0 (axis -2) or 1 (axis -1)")
            w = wvar
    # the default order: the compact stored shape of the definition -- but where wvar != var with f's own length on var, of which index 0
    # alone is stored, because an operand lies inside the orders
    compact = list(shape)
    if not comp:
        compact[w] = shape[w] + 1
    elif w != v:
        compact[w] = shape[w] + shape[v] - 1
    if n is None:
        if out is not None:
            if out.dim() < planes + rank:
                raise TaylorError(f"{what}: out has shape {tuple(out.shape)}; the result has {rank} series ax{'is' if rank == 1 else 'es'}")
            order = tuple(out.shape[-rank:])
        else:
            order = tuple(compact)
    else:
        import operator

        try:
            order = (operator.index(n),) if rank == 1 else tuple(operator.index(k) for k in n)
        except TypeError:
            raise TypeError(f"{what}: n must be {'an integer' if rank == 1 else 'a pair of integers'}, got {n!r}") from None
        if len(order) != rank:
            raise TaylorError(f"{what}: n = {n!r}; the order of a bivariate result is a pair (n0, n1)")
    on = f" on axis {w - 2}" if rank == 2 else ""
    if order[w] < 2:
        raise TaylorError(f"{what}: the result has {order[w]} coefficient{on} (c + m * x needs two: a substitution at one coefficient is the "
                          "constant one, not a linear one)")
    if any(k < 1 for k in order):
        raise TaylorError(f"{what}: n = {order if rank == 2 else order[0]} (the result has no coefficients)")
    if any(s > k for s, k in zip(shape, order)):
        raise TaylorError(f"{what}: {aname} has {shape if rank == 2 else shape[0]} coefficients, the result n = {order if rank == 2 else order[0]} "
                          "(an operand is longer than the truncation order)")
    count = order[0] * order[-1] if rank == 2 else order[0]
    if count > limit:
        raise TaylorError(f"{what}: n = {order if rank == 2 else order[0]} exceeds the limit of {limit} coefficients per "
                          f"{'item' if rank == 2 else 'series'} of this version")
    named = [(aname, a.shape[planes:a.dim() - rank]), ("c", c.shape[planes:]), ("m", m.shape[planes:])]
    try:
        batch = tuple(torch.broadcast_shapes(*[s for _, s in named]))
    except RuntimeError:
        raise TaylorError(f"{what}: the batch shapes do not broadcast: " + ", ".join(f"{k} has {tuple(s)}" for k, s in named)
                          + " (c and m have the batch shape: one scalar per item)") from None
    if out is not None:
        if out.dim() < planes + rank or tuple(out.shape[-rank:]) != order:
            raise TaylorError(f"{what}: out has shape {tuple(out.shape)}; the result has n = {order if rank == 2 else order[0]} coefficients per item")
        if tuple(out.shape[planes:out.dim() - rank]) != batch:
            raise TaylorError(f"{what}: out has batch shape {tuple(out.shape[planes:out.dim() - rank])}; the operands broadcast to {batch}")
    if torch.is_grad_enabled():
        for t, k in ((a, aname), (c, "c"), (m, "m")):
            if t.requires_grad:
                raise TaylorError(f"{what}: {k} requires grad, and {op.label} has no autograd in this version; pass {k}.detach() or call "
                                  "under torch.no_grad() (nothing is detached silently)")
    named = (("x", aname, a, shape), ("second", "c", c, ()), ("cs", "m", m, ()))
    return _launch(what, op, call, named, out, batch, order, ((), (v, w)[:int(op.var)], ()))


NEGBIN_MAX = {0: 8192, 1: 4096}  # gft_series_args.hpp SERIES_NEGBIN_MAX / _IV, by the planes: the limit on 3 * degree_p1 + order


def run_negbinomial(call, a, var, x, p, ls, degree_p1=None, out=None):
    """One call of gft[i]_series[2]_observe_negbinomial: ``a`` the operand, ``var`` the axis at rank 2, ``x`` and ``p`` one scalar per
    item each, ``ls`` the row ``[B..., order + 1]``.  The checks come in ``run_chain``'s order."""
    import torch

    op, (module, rank, planes, limit, _raw, _kind) = MORE_OPS["observe_negbinomial"], call
    what = f"{module}.{op.label}"
    over_text = _rank_rules(rank)[2]
    for t, w in ((a, "a"), (x, "x"), (p, "p"), (ls, "ls"), (out, "out")):
        if t is None and w == "out":
            continue
        w = f"{what}: {w}"
        _check(torch, t, w, planes)
        if t is a or t is out:
            _axes(rank, t, w, planes)
    if ls.dim() < 1 + planes:
        raise TaylorError(f"{what}: ls has no axis of entries; it is [{'2, ' if planes else ''}B..., order + 1]")
    if ls.shape[-1] > 1 and ls.stride(-1) != 1:
        raise TaylorError(f"{what}: ls: the last axis (the entries) has stride {ls.stride(-1)}; it must have unit stride")
    shape = tuple(a.shape[-rank:])
    count = shape[0] * shape[-1] if rank == 2 else shape[0]
    if count > limit:
        raise TaylorError(over_text.format(what=what, shape=shape, count=count, limit=limit).replace(": x has", ": a has"))
    axis = -1
    if rank == 2:
        from .series2 import _var

        axis = _var(what, var, "the variable the observation acts on is 0 (axis -2) or 1 (axis -1)") - 2
    length, nls, on = shape[axis], int(ls.shape[-1]), f" on axis {axis}" if rank == 2 else ""
    if nls == 0:
        raise TaylorError(f"{what}: ls holds no entry (a row of order K has K + 1 >= 1 entries)")
    order = nls - 1
    d = length - order if degree_p1 is None else _count(what, "degree_p1", degree_p1)
    if d < 3:
        raise TaylorError(f"{what}: degree_p1 = {d} (the result needs at least three coefficients{on}: degree_p1 >= 3"
                          + (f"; the default is {length} - order)" if degree_p1 is None else ")"))
    if d + order > length:
        raise TaylorError(f"{what}: degree_p1 + order = {d} + {order}, but a has {length} stored coefficients{on} (every pass takes one: "
                          f"degree_p1 + order <= {length})")
    if 3 * d + order > NEGBIN_MAX[planes]:
        raise TaylorError(f"{what}: 3 * degree_p1 + order = 3 * {d} + {order} exceeds the limit of {NEGBIN_MAX[planes]} of this operation")
    rshape = (d,) if rank == 1 else ((d, min(shape[1], d)) if axis == -2 else (min(shape[0], d), d))
    named = [("a", a.shape[planes:a.dim() - rank]), ("x", x.shape[planes:]), ("p", p.shape[planes:]), ("ls", ls.shape[planes:-1])]
    try:
        batch = tuple(torch.broadcast_shapes(*[s for _, s in named]))
    except RuntimeError:
        raise TaylorError(f"{what}: the batch shapes do not broadcast: " + ", ".join(f"{n} has {tuple(s)}" for n, s in named)
                          + " (x and p have the batch shape, ls the batch shape and one last axis of order + 1 entries)") from None
    if out is not None:
        if out.dim() < planes + rank or tuple(out.shape[-rank:]) != rshape:
            raise TaylorError(f"{what}: out has shape {tuple(out.shape)}; the result has {rshape} coefficients per item (degree_p1 = {d}{on})")
        if tuple(out.shape[planes:out.dim() - rank]) != batch:
            raise TaylorError(f"{what}: out has batch shape {tuple(out.shape[planes:out.dim() - rank])}; the operands broadcast to {batch}")
    if torch.is_grad_enabled():
        for t, w in ((a, "a"), (x, "x"), (p, "p"), (ls, "ls")):
            if t.requires_grad:
                raise TaylorError(f"{what}: {w} requires grad, and observe_negbinomial has no autograd in this version; pass {w}.detach() or "
                                  "call under torch.no_grad() (nothing is detached silently)")
    named = (("x", "a", a, shape), ("second", "x", x, ()), ("p", "p", p, ()), ("cs", "ls", ls, (nls,)))
    return _launch(what, op, call, named, out, batch, rshape, ((), (var,), (nls, d)))


def run_lah_row(call, p, order, out=None):
    """One call of gft[i]_series_lah_row: ``p`` one scalar per item, the result ``[B..., order + 1]``."""
    import torch

    op, (module, _rank, planes, limit, _raw, _kind) = MORE_OPS["lah_row"], call
    what = f"{module}.{op.label}"
    _check(torch, p, f"{what}: p", planes)
    if out is not None:
        _check(torch, out, f"{what}: out", planes)
        _axes(1, out, f"{what}: out", planes)
    order = _count(what, "order", order)
    if order < 0:
        raise TaylorError(f"{what}: order = {order} (a row has order + 1 >= 1 entries)")
    if order + 1 > limit:
        raise TaylorError(f"{what}: order + 1 = {order + 1} exceeds the limit of {limit} coefficients per series of this version")
    batch = tuple(p.shape[planes:])
    if out is not None:
        if out.shape[-1] != order + 1:
            raise TaylorError(f"{what}: out has shape {tuple(out.shape)}; the result has {order + 1} entries per item (order = {order})")
        if tuple(out.shape[planes:-1]) != batch:
            raise TaylorError(f"{what}: out has batch shape {tuple(out.shape[planes:-1])}; p has {batch}")
    if torch.is_grad_enabled() and p.requires_grad:
        raise TaylorError(f"{what}: p requires grad, and lah_row has no autograd in this version; pass p.detach() or call under "
                          "torch.no_grad() (nothing is detached silently)")
    return _launch(what, op, call, (("x", "p", p, ()),), out, batch, (order + 1,), ((), (), (order,)))
