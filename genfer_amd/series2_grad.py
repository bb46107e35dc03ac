"""Differentiable batched bivariate series: ``mul``, ``div``, ``exp``, ``log``, ``compose``, ``pow`` and the observation ops
``derivative``, ``taylor_expansion_of_coeff``, ``shift_down``, ``evaluate_all_one`` with the signatures, the
operand layout and the forward bits of ``genfer_amd.series2``, recording a ``grad_fn`` for torch's autograd.

``series2`` is the raw layer and refuses an operand that requires grad; this module is its differentiable twin, as
``interval_series2`` is its interval twin.  With grad mode off, or with no operand that requires grad, a call here IS the call of
``series2`` (``out=`` included).  Otherwise the forward pass runs the same launch on the detached operands and the backward pass is
a short sequence of ``series2``'s own calls on detached tensors, around ``series2.corr`` -- the adjoint of the truncated product,
``<mul(x, y, n), g> = <x, corr(g, y)>`` -- and, for ``compose``, the transposed Horner loop ``series2._compose_adj`` (one launch).
With ``n`` the shape of the result's series axes, ``one`` the item ``[[1.0]]`` and ``gz`` the incoming gradient (made contiguous
first when its last stride is not 1, as ``z.sum().backward()`` hands it over):

    mul      gx = corr(gz, y, x.shape[-2:]);  gy = corr(gz, x, y.shape[-2:])
    div      (r = x / y)  u = corr(gr, div(one, y, n), n);  gx = u[..., :nx0, :nx1];  gy = -corr(u, r, y.shape[-2:])
    exp      (e = exp(x)) gx = corr(ge, e, x.shape[-2:])
    log      gx = corr(gl, div(one, x, n), x.shape[-2:])
    pow      e == 0: zeros;  else gx = e * corr(gp, pow(x, e - 1, n), x.shape[-2:])
    compose  gf = _compose_adj(gh, g, var, f.shape[-2:]);  gg = corr(gh, compose(fp, g, var, n), g.shape[-2:]), where fp is the
             derivative of f along axis var: slice i of f times i, shifted down one (zeros of f's shape when f has one slice)

Every gradient is then reduced over the broadcast batch axes with ``sum_to_size`` (torch's order of additions); everything before
that carries the bits of the calls above.  Only the gradients that are asked for are computed.  First derivatives only
(``once_differentiable``), float64 only; ``out=`` cannot be combined with an operand that requires grad, and a ``seed`` never
carries a gradient (it is ``exp(x[..., 0, 0])`` / ``ln(x[..., 0, 0])`` by contract: the gradient flows to ``x``).

    >>> from genfer_amd import series2_grad as s2g
    >>> w = torch.rand(4, 6, dtype=torch.float64, device="cuda", requires_grad=True)
    >>> s2g.compose(w, g, var=1).sum().backward()   # w.grad: the transposed Horner loop, summed over the batch of g
"""
from __future__ import annotations

from . import series2
from .series import _exponent, _tracked


def _autograd():
    """The torch.autograd.Function of every operation (one set for both ranks: _series_autograd.py)."""
    from ._series_autograd import functions

    return functions("series2_grad", 2)


def mul(x, y, n=None, out=None):
    """``series2.mul``, differentiable in ``x`` and ``y``."""
    if _tracked("series2_grad.mul", (x, y), out):
        return _autograd().Mul.apply(x, y, n)
    return series2.mul(x, y, n, out)


def div(x, y, n=None, out=None):
    """``series2.div``, differentiable in ``x`` and ``y``."""
    if _tracked("series2_grad.div", (x, y), out):
        return _autograd().Div.apply(x, y, n)
    return series2.div(x, y, n, out)


def exp(x, n=None, seed=None, out=None):
    """``series2.exp``, differentiable in ``x`` (never in ``seed``)."""
    if _tracked("series2_grad.exp", (x,), out, seed):
        return _autograd().Exp.apply(x, n, seed)
    return series2.exp(x, n, seed, out)


def log(x, n=None, seed=None, out=None):
    """``series2.log``, differentiable in ``x`` (never in ``seed``)."""
    if _tracked("series2_grad.log", (x,), out, seed):
        return _autograd().Log.apply(x, n, seed)
    return series2.log(x, n, seed, out)


def compose(f, g, var=0, n=None, out=None):
    """``series2.compose``, differentiable in ``f`` (the transposed Horner loop) and ``g``."""
    if _tracked("series2_grad.compose", (f, g), out):
        return _autograd().Compose.apply(f, g, series2._var("series2_grad.compose", var), n)
    return series2.compose(f, g, var, n, out)


def pow(x, e, n=None, out=None):  # noqa: A001 (the reference's name)
    """``series2.pow``, differentiable in ``x``."""
    if _tracked("series2_grad.pow", (x,), out):
        return _autograd().Pow.apply(x, _exponent("series2_grad.pow", e, div="series2_grad.div"), n)
    return series2.pow(x, e, n, out)


# ---- the observation ops: linear maps, their adjoints torch indexing around series2's own calls ------------------------------
#     derivative, taylor_expansion_of_coeff   gx[k + j] = gz[j] * factor_j along axis var (the factors: the op of ones), gx[< k] = +0.0
#     shift_down                              gx[i] = gz[0] for i <= k, gx[k + j] = gz[j] for j >= 1, along axis var
#     evaluate_all_one                        gz broadcast over the item


def derivative(x, var, k, out=None):
    """``series2.derivative``, differentiable in ``x``."""
    if _tracked("series2_grad.derivative", (x,), out):
        return _autograd().Derivative.apply(x, var, k)
    return series2.derivative(x, var, k, out)


def taylor_expansion_of_coeff(x, var, k, out=None):
    """``series2.taylor_expansion_of_coeff``, differentiable in ``x``."""
    if _tracked("series2_grad.taylor_expansion_of_coeff", (x,), out):
        return _autograd().Coeff.apply(x, var, k)
    return series2.taylor_expansion_of_coeff(x, var, k, out)


def shift_down(x, var, k, out=None):
    """``series2.shift_down``, differentiable in ``x``."""
    if _tracked("series2_grad.shift_down", (x,), out):
        return _autograd().ShiftDown.apply(x, var, k)
    return series2.shift_down(x, var, k, out)


def evaluate_all_one(x, out=None):
    """``series2.evaluate_all_one``, differentiable in ``x``."""
    if _tracked("series2_grad.evaluate_all_one", (x,), out):
        return _autograd().EvalOne.apply(x)
    return series2.evaluate_all_one(x, out)
