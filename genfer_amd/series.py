"""Batched univariate series on float64 device tensors: ``mul``, ``div``, ``exp``, ``log``, ``compose``, ``pow``, the transposed
product ``corr`` and the observation ops ``derivative``, ``taylor_expansion_of_coeff``, ``shift_down``, ``evaluate_all_one``
(``gft_series_*``), all but ``corr`` differentiable by torch's autograd, and the fused Poisson observation chain ``observe_chain`` (no
autograd).

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

from ._series_call import Call, _lib  # noqa: F401  (one declared library for the four modules)
from ._series_call import run as _run
from .taylor import TaylorError

MAX_N = 4096  # gft_series.hpp SERIES_MAX_N: the limit of this version

_CALL = Call("series", 1, 0, MAX_N, raw=False)  # rank 1, one plane; autograd is this module's own (_tracked)


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


def mul(x, y, n=None, out=None):
    """``z[b] = x[b] * y[b]`` truncated at order ``n`` (default ``max(nx, ny)``): the general product ``mul_1d``."""
    if _tracked("series.mul", (x, y), out):
        return _autograd().Mul.apply(x, y, n)
    return _run(_CALL, "mul", x, y, n, out)


def div(x, y, n=None, out=None):
    """``r[b] = x[b] / y[b]`` to order ``n`` (default ``max(nx, ny)``): the general division recurrence."""
    if _tracked("series.div", (x, y), out):
        return _autograd().Div.apply(x, y, n)
    return _run(_CALL, "div", x, y, n, out)


def exp(x, n=None, seed=None, out=None):
    """``exp(x[b])`` to order ``n`` (default ``nx``).  ``seed``: ``exp(x[b, 0])`` per item (a tensor of the batch shape); with
    the host libm's values the result carries the reference's bits.  ``None``: formed on the device (a few ulps from libm)."""
    if _tracked("series.exp", (x,), out, seed):
        return _autograd().Exp.apply(x, n, seed)
    return _run(_CALL, "exp", x, seed, n, out)


def log(x, n=None, seed=None, out=None):
    """``log(x[b])`` to order ``n`` (default ``nx``).  ``seed``: ``ln(x[b, 0])`` per item; ``None``: formed on the device (only
    coefficient 0 depends on it)."""
    if _tracked("series.log", (x,), out, seed):
        return _autograd().Log.apply(x, n, seed)
    return _run(_CALL, "log", x, seed, n, out)


def compose(f, g, n=None, out=None):
    """``f[b](g[b])`` truncated at order ``n`` (default ``max(nf, ng)``): Horner over the coefficients of ``f`` with the general
    product at every step, ``res = res * g + f[i]`` for ``i = nf-2 .. 0`` from ``res = [0.0 + f[nf-1]]`` — ``subst_var``'s general
    path without its zero / linear shortcuts, the row resident in LDS across the steps.  About ``nf * n**2 / 2`` multiply-adds per
    item, on one workgroup at most."""
    if _tracked("series.compose", (f, g), out):
        return _autograd().Compose.apply(f, g, None, n)
    return _run(_CALL, "compose", f, g, n, out)


def corr(g, y, m=None, out=None):
    """The transposed product, the adjoint of ``mul``: ``<mul(x, y), g> = <x, corr(g, y)>``.  ``g`` has ``ng`` coefficients, ``y``
    has ``ny <= ng``, the result ``m <= ng`` (default ``ng``)::

        c[b, i] = 0.0 + sum_k g[b, k] * y[b, k - i],   k descending from min(ng - 1, i + ny - 1) to i

    multiply and add rounded separately, only stored coefficients entering a sum: bit for bit ``mul(flip(g), y)`` at index
    ``ng - 1 - i``.  ``out`` may be ``g`` itself, never ``y``.  Not differentiable itself (the backward passes are built from it)."""
    return _run(_CALL, "corr", g, y, m, out)


def _compose_adj(gh, g, nf, out=None):
    """The transposed Horner loop: the gradient of ``compose(f, g, n)`` with respect to ``f`` (``nf`` coefficients) from the
    gradient ``gh`` of the composition (``n`` coefficients) -- ``a = gh[:l_0]; out[0] = a[0];`` then ``a = corr(a, g, l_{i+1});
    out[i + 1] = a[0]`` at the compact lengths ``l_i = min(1 + (nf - 1 - i)(ng - 1), n)``, in one launch."""
    return _run(_CALL, "compose_adj", gh, g, nf, out)


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
    return _run(_CALL, "pow", x, None, n, out, scalar=e)


# ---- the observation ops: derivative, taylor_expansion_of_coeff, shift_down, evaluate_all_one --------------------------------
# One operand, an order k on one axis; the result is k shorter there (include/gftaylor.h states the loops).


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


def derivative(x, k, out=None):
    """The ``k``-th derivative's coefficients: ``out[b, j] = x[b, k + j] * ff_j`` for ``j < nx - k``, one rounding each, with the
    reference's running-product factors ``ff_0 = k!``, ``ff_{j+1} = ff_j * ((k + j + 1) / (j + 1))`` (the quotient rounded first)."""
    if _tracked("series.derivative", (x,), out):
        return _autograd().Derivative.apply(x, None, k)
    return _run(_CALL, "derivative", x, out=out, scalar=k)


def taylor_expansion_of_coeff(x, k, out=None):
    """The expansion of coefficient ``k``: ``out[b, 0] = x[b, k]`` and ``out[b, j] = x[b, k + j] * f_j`` with ``f_0 = 1``,
    ``f_j = f_{j-1} * ((k + j) / j)`` -- ``derivative`` without its factor ``k!``."""
    if _tracked("series.taylor_expansion_of_coeff", (x,), out):
        return _autograd().Coeff.apply(x, None, k)
    return _run(_CALL, "taylor_expansion_of_coeff", x, out=out, scalar=k)


def shift_down(x, k, out=None):
    """The coefficients moved down by ``k``, those pushed out gathered at 0: ``out[b, 0] = x[b, k] + (0.0 + x[b, 0] + ... +
    x[b, k - 1])`` (ascending; with ``nx == k + 1`` the ascending sum of all of them) and ``out[b, j] = x[b, k + j]``."""
    if _tracked("series.shift_down", (x,), out):
        return _autograd().ShiftDown.apply(x, None, k)
    return _run(_CALL, "shift_down", x, out=out, scalar=k)


def evaluate_all_one(x, out=None):
    """The series at ``t = 1``: ``0.0 + x[b, 0] + x[b, 1] + ...``, one ascending chain per item; the result has the batch shape."""
    if _tracked("series.evaluate_all_one", (x,), out):
        return _autograd().EvalOne.apply(x)
    return _run(_CALL, "evaluate_all_one", x, out=out)


def observe_chain(a, x, cs, degree_p1=None, out=None):
    """The fused Poisson observation chain, ``observe k ~ Poisson(rate * X)`` with ``k = cs.shape[-1]`` steps in one launch.  Step ``t``
    is ``(derivative(1).truncate(d_t) * var(x, d_t)) * cs[..., t]`` at ``d_t = degree_p1 + (nsteps - 1 - t)``, each step on the one
    before (``gft_observe_chain``'s unfolding; ``include/gftaylor.h`` states the loops).  ``x``: one scalar per item (the batch shape),
    or ``None`` for a continuous rate, where a step is ``derivative(1).truncate(d_t) * cs[..., t]``.  ``cs``: ``[B..., nsteps]``, unit
    stride on its last axis.  ``x`` and ``cs`` broadcast against the batch.  ``degree_p1`` (default ``L - nsteps``, ``L`` the stored
    length) is the result's length; ``degree_p1 >= 2`` and ``degree_p1 + nsteps <= L``.  No autograd in this version."""
    from ._series_call import run_chain

    return run_chain(_CALL, a, None, x, cs, degree_p1, out)


def lah_row(p, order, out=None):
    """The row of scaled Lah numbers ``observe k ~ NegBinomial(X, p)`` sums with (generating_function.rs:713-730): ``p`` is ``[B...]``
    (any strides), the result ``[B..., order + 1]``.  ``row_0 = [1]`` and ``row_d[i] = ((1 - p) / d) * (row_{d-1}[i] * (d + i - 1) +
    row_{d-1}[i - 1])`` with the absent entries zero, multiplied by and added all the same.  One launch; no autograd."""
    from ._series_call import run_lah_row

    return run_lah_row(_CALL, p, order, out)


def observe_negbinomial(a, x, p, ls, degree_p1=None, out=None):
    """The fused negative-binomial observation ``observe k ~ NegBinomial(X, p)`` with ``k = ls.shape[-1] - 1`` in one launch: ``a`` is
    the inner generating function evaluated at ``p * x`` to ``degree_p1 + k`` coefficients, ``x`` and ``p`` one scalar per item,
    ``ls`` the row ``[B..., k + 1]`` (usually ``lah_row(p, k)``).  Pass ``i`` scales coefficient ``j`` of the ``i``-th derivative by
    ``p ** j``, multiplies by ``(p * x + p * t) ** i``, scales by ``ls[..., i]`` and adds (``include/gftaylor.h`` states the loops).
    ``degree_p1`` (default ``L - k``) is the result's length; ``degree_p1 >= 3``, ``degree_p1 + k <= L`` and
    ``3 * degree_p1 + k <= 8192``.  No autograd in this version."""
    from ._series_call import run_negbinomial

    return run_negbinomial(_CALL, a, None, x, p, ls, degree_p1, out)


def mul_linear(a, c, m, n=None, out=None):
    """``a`` times the linear series ``c + m * t`` as the reference multiplies by one (``mul_linear``; ``include/gftaylor.h`` states the
    loop): ``out[j] = a[j-1] * m + c * a[j]``, the sum and the second product absent where ``c == 0`` (by value, per item).  ``c``, ``m``:
    one scalar per item (the batch shape; they broadcast against it).  ``n`` (default ``L + 1``, ``L`` the stored length)
    is the result's order.  No autograd in this version."""
    from ._series_call import run_linear

    return run_linear(_CALL, "mul_linear", a, None, None, c, m, n, out)


def compose_linear(f, c, m, n=None, out=None):
    """``f(c + m * t)`` as the reference substitutes an affine series (``subst_var``'s linear paths; ``include/gftaylor.h`` states the
    loops): where ``c == 0`` (by value, per item) coefficient ``i`` times ``m^i`` from a running table, else Horner's loop with
    ``mul_linear`` as its product.  ``c``, ``m``: one scalar per item.  ``n`` (default: ``f``'s stored length) is the
    result's order.  One launch, about ``nf * n`` multiply-adds per item; ``compose(f, [c, m])`` has other bits and ``nf * n^2 / 2``.
    No autograd in this version."""
    from ._series_call import run_linear

    return run_linear(_CALL, "compose_linear", f, None, None, c, m, n, out)


# ---- autograd (the Functions: _series_autograd.py) ---------------------------------------------------------------------------

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


def _autograd():
    """The torch.autograd.Function of every operation (one set for both ranks: _series_autograd.py)."""
    from ._series_autograd import functions

    return functions("series", 1)


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
