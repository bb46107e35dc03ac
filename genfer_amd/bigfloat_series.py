"""Batched univariate series on BigFloat device tensors: ``mul``, ``div``, ``exp``, ``log``, ``compose``, ``pow``
(``gftb_series_*``), the ``BigFloat`` third of ``genfer_amd.series`` beside float64 and ``interval_series``.

A BigFloat tensor is float64 and stacked ``[2, B..., n]`` = (factor, exponent) along its first axis: a coefficient is
``factor * 2**exponent`` with the factor in ±[1, 2), or 0 with exponent 0, or non-finite, and the exponent an integral double with
``|e| < 2**52`` (src/number/big_float.rs; ``encode`` makes such tensors from float64 values, ``decode`` turns them back).  The last
axis is the series (unit stride), the axes between are batch axes and broadcast by torch's rules.  The plane axis may have any
positive stride; 0 is refused, because a factor plane cannot be its own exponent plane.  Seeds of ``exp`` / ``log`` are ``[2, B...]``.
Item ``b`` is the ``TaylorPoly<BigFloat>`` of one variable at truncation order ``n <= 2048``.  Per item the results are the
reference's *general* algorithms in BigFloat arithmetic -- every factor and exponent with the oracle's bits, including the additions
of zero the reference performs (``0 + b`` drops ``b`` at exponent <= -1024) -- and none of the operators' shortcuts.  Exponent
differences of ``2**31`` or more are unsupported, and inputs are not scanned: values outside the contract give unspecified values.
This is a raw layer without autograd; the call is ordered on torch's current stream and does not wait.

    >>> from genfer_amd import bigfloat_series as bfs
    >>> x = bfs.encode(v, exponent_offset=-3000)   # v: [B, n] float64; the values v * 2**-3000, far outside the f64 range
    >>> z = bfs.mul(x, y)                          # x, y: [2, B, n] float64 on the GPU
    >>> e = bfs.exp(x, seed=s)                     # s: [2, B], the BigFloat exp of coefficient 0
    >>> p = bfs.pow(x, 5)
    >>> bfs.decode(z)                              # float64 values, as BigFloat::to_f64 makes them
"""
from __future__ import annotations

from ._series_call import Call
from .series import FORMS, _exponent, _run, last_form, set_form  # noqa: F401  (one library, one form option, one last form)

MAX_N = 2048  # gft_series_args.hpp SERIES_MAX_N_IV: two planes, the interval footprint

_CALL = Call("bigfloat_series", 1, 1, MAX_N, raw=True, elem="bigfloat")


def mul(x, y, n=None, out=None):
    """``z[b] = x[b] * y[b]`` truncated at order ``n`` (default ``max(nx, ny)``): the general product, every sum formed from 0 and
    added onto a zero as ``mul_rec`` does."""
    return _run(_CALL, "mul", x, y, n, out)


def div(x, y, n=None, out=None):
    """``r[b] = x[b] / y[b]`` to order ``n`` (default ``max(nx, ny)``): the general division recurrence in BigFloat arithmetic."""
    return _run(_CALL, "div", x, y, n, out)


def exp(x, n=None, seed=None, out=None):
    """``exp(x[b])`` to order ``n`` (default ``nx``).  ``seed``: ``BigFloat::exp`` of coefficient 0 per item, ``[2, B...]``; with a
    host libm's values the result carries the oracle's bits.  ``None``: formed on the device (a few ulps from a host's)."""
    return _run(_CALL, "exp", x, seed, n, out)


def log(x, n=None, seed=None, out=None):
    """``log(x[b])`` to order ``n`` (default ``nx``).  ``seed``: ``BigFloat::log`` of coefficient 0 per item, ``[2, B...]``;
    ``None``: formed on the device (only coefficient 0 depends on it)."""
    return _run(_CALL, "log", x, seed, n, out)


def compose(f, g, n=None, out=None):
    """``f[b](g[b])`` truncated at order ``n`` (default ``max(nf, ng)``): Horner over the coefficients of ``f`` with ``mul``'s product
    at every step, as ``series.compose``; one coefficient of ``f`` gives ``0 + f``."""
    return _run(_CALL, "compose", f, g, n, out)


def pow(x, e, n=None, out=None):  # noqa: A001 (the reference's name)
    """``x[b] ** e`` truncated at order ``n`` (default ``nx``) for an integer ``0 <= e < 2**32``: the reference's
    square-and-multiply over ``mul`` at compact lengths, from the unit series.  ``e = 0`` gives ``[{1, 0}, {0, 0}, ...]``."""
    return _run(_CALL, "pow", x, None, n, out, scalar=_exponent("bigfloat_series.pow", e, div="bigfloat_series.div"))


# ---- float64 values <-> BigFloat planes, in torch on any device (genfer_amd.bigfloat.encode / decode are the numpy statements) ----


def encode(t, exponent_offset=0):
    """``[2, *t.shape]``: the (factor, exponent) planes of the float64 tensor ``t`` as big_float.rs ``normalize`` makes them, every
    exponent raised by ``exponent_offset``: zeros of either sign give ``{+0, 0}``, non-finite values keep the exponent
    ``exponent_offset``, subnormals are rescaled exactly."""
    import torch

    if t.dtype != torch.float64:
        raise TypeError(f"bigfloat_series.encode: the tensor is {t.dtype}; only torch.float64 is accepted (no implicit conversion)")
    m, e = torch.frexp(t)  # t = m * 2**e, |m| in [0.5, 1): exact, subnormals included
    off = float(exponent_offset)
    fin, zero = torch.isfinite(t), t == 0.0
    f = torch.where(fin, m * 2.0, t)
    e = torch.where(fin, e.to(torch.float64) - 1.0 + off, torch.full_like(t, off))
    nought = torch.zeros_like(t)
    return torch.stack([torch.where(zero, nought, f), torch.where(zero, nought, e)])


def decode(t):
    """The float64 values of a BigFloat tensor ``[2, ...]`` as ``BigFloat::to_f64`` makes them: ``factor * powi(2, exponent)`` with
    ``powi(2, n)`` exactly ``2**n`` for ``-1023 <= n <= 1023``, ``+0`` below and ``+inf`` above (so ``inf * 0`` is NaN, as there)."""
    import torch

    if t.dtype != torch.float64 or t.dim() < 1 or t.shape[0] != 2:
        raise TypeError("bigfloat_series.decode: expected a float64 tensor stacked [2, ...] = (factor, exponent)")
    f, n = t[0], t[1]
    p = torch.ldexp(torch.ones_like(f), torch.clamp(n, -1024.0, 1024.0).to(torch.int64))
    p = torch.where(n <= -1024.0, torch.zeros_like(f), torch.where(n >= 1024.0, torch.full_like(f, float("inf")), p))
    return f * p
