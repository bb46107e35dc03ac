"""The torch.autograd.Functions of the batched series, one set for both ranks: ``functions("series", 1)`` serves ``series``,
``functions("series2_grad", 2)`` serves ``series2_grad``.

Every vector-Jacobian product is a sequence of the raw module's own calls (``series`` at rank 1, ``series2`` at rank 2) on detached
tensors; ``corr`` carries the order of its sums, so a gradient's bits are pinned up to the reduction over broadcast batch axes
(sum_to_size: torch's order).  Item shapes come from ``shape[-rank:]``; ``var`` is None at rank 1, where the one series axis is -1.
The observation ops are linear maps; their adjoints are torch indexing around the same calls.
"""
from __future__ import annotations

import types

from ._series_call import Call, run

_built = {}


def functions(name, rank):
    """The Functions of module ``name`` (its name in messages) at ``rank``, built on first use: the modules import without torch."""
    if (name, rank) in _built:
        return _built[(name, rank)]
    import torch
    from torch.autograd.function import once_differentiable

    from . import series, series2

    raw = series if rank == 1 else series2
    call = Call(name, rank, 0, raw._CALL.limit, False)  # (the operands arrive detached: nothing to refuse)
    call1 = call._replace(rank=1)
    vargs = (lambda var: ()) if rank == 1 else (lambda var: (var,))  # var in the raw module's signatures

    def item(shape):  # an order as the raw module takes it: an int at rank 1, a pair at rank 2
        return shape[-1] if rank == 1 else tuple(shape[-2:])

    def axis_of(var):
        return -1 if var is None else var - 2

    def unit_stride(g):  # z.sum().backward() hands over an expanded scalar: stride 0 on the series axes
        return g if g.shape[-1] == 1 or g.stride(-1) == 1 else g.contiguous()

    def one(t):
        return torch.ones((1,) * rank, dtype=torch.float64, device=t.device)

    class Mul(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y, n):
            x, y = x.detach(), y.detach()
            ctx.save_for_backward(x, y)
            return run(call, "mul", x, y, n)

        @staticmethod
        @once_differentiable
        def backward(ctx, gz):
            x, y = ctx.saved_tensors
            gz = unit_stride(gz)
            gx = raw.corr(gz, y, item(x.shape)).sum_to_size(x.shape) if ctx.needs_input_grad[0] else None
            gy = raw.corr(gz, x, item(y.shape)).sum_to_size(y.shape) if ctx.needs_input_grad[1] else None
            return gx, gy, None

    class Div(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y, n):
            x, y = x.detach(), y.detach()
            r = run(call, "div", x, y, n)
            ctx.save_for_backward(r, y)
            ctx.shapes = (x.shape, y.shape)
            return r

        @staticmethod
        @once_differentiable
        def backward(ctx, gr):
            r, y = ctx.saved_tensors
            xs, ys = ctx.shapes
            n = item(r.shape)
            u = raw.corr(unit_stride(gr), raw.div(one(y), y, n), n)  # the gradient of the dividend at the full shape
            gx = u[(...,) + tuple(slice(0, s) for s in xs[-rank:])].sum_to_size(xs) if ctx.needs_input_grad[0] else None
            gy = (-raw.corr(u, r, item(ys))).sum_to_size(ys) if ctx.needs_input_grad[1] else None
            return gx, gy, None

    class Exp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, n, seed):
            x = x.detach()
            e = run(call, "exp", x, seed, n)
            ctx.save_for_backward(e)
            ctx.shape = x.shape
            return e

        @staticmethod
        @once_differentiable
        def backward(ctx, ge):
            (e,) = ctx.saved_tensors
            return raw.corr(unit_stride(ge), e, item(ctx.shape)).sum_to_size(ctx.shape), None, None

    class Log(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, n, seed):
            x = x.detach()
            ctx.save_for_backward(x)
            return run(call, "log", x, seed, n)

        @staticmethod
        @once_differentiable
        def backward(ctx, gl):
            (x,) = ctx.saved_tensors
            n = item(gl.shape)
            return raw.corr(unit_stride(gl), raw.div(one(x), x, n), item(x.shape)).sum_to_size(x.shape), None, None

    class Pow(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, e, n):
            x = x.detach()
            ctx.save_for_backward(x)
            ctx.e = e
            return run(call, "pow", x, None, n, scalar=e)

        @staticmethod
        @once_differentiable
        def backward(ctx, gp):
            (x,) = ctx.saved_tensors
            if ctx.e == 0:
                return torch.zeros_like(x), None, None
            n = item(gp.shape)
            return (ctx.e * raw.corr(unit_stride(gp), raw.pow(x, ctx.e - 1, n), item(x.shape))).sum_to_size(x.shape), None, None

    class Compose(torch.autograd.Function):
        @staticmethod
        def forward(ctx, f, g, var, n):
            f, g = f.detach(), g.detach()
            ctx.save_for_backward(f, g)
            ctx.var = var
            return run(call, "compose", f, g, n, var=var)

        @staticmethod
        @once_differentiable
        def backward(ctx, gh):
            f, g = ctx.saved_tensors
            var, ax = ctx.var, axis_of(ctx.var)
            gh = unit_stride(gh)
            n = item(gh.shape)
            gf = gg = None
            if ctx.needs_input_grad[0]:
                gf = raw._compose_adj(gh, g, *vargs(var), item(f.shape)).sum_to_size(f.shape)
            if ctx.needs_input_grad[1]:  # h = f(g): dh = (df / dvar)(g) * dg
                slices = f.shape[ax]
                if slices > 1:
                    i = torch.arange(1, slices, dtype=torch.float64, device=f.device)
                    fp = f.narrow(ax, 1, slices - 1) * i.reshape((-1,) + (1,) * (-1 - ax))
                else:
                    fp = torch.zeros_like(f)
                gg = raw.corr(gh, raw.compose(fp, g, *vargs(var), n), item(g.shape)).sum_to_size(g.shape)
            return gf, gg, None, None

    def scaled(cls_name, op):
        class Scaled(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, var, k):
                x = x.detach()
                ctx.var, ctx.shape = var, x.shape
                z = run(call, op, x, scalar=k, var=var)
                ctx.k = x.shape[axis_of(var)] - z.shape[axis_of(var)]
                return z

            @staticmethod
            @once_differentiable
            def backward(ctx, gz):  # gx[k + j] = gz[j] * factor_j, the factors the forward op of ones; gx[< k] = +0.0
                ax, k = axis_of(ctx.var), ctx.k
                ln = ctx.shape[ax]
                fac = run(call1, op, torch.ones(ln, dtype=torch.float64, device=gz.device), scalar=k)
                gx = torch.zeros(ctx.shape, dtype=torch.float64, device=gz.device)
                gx.narrow(ax, k, ln - k).copy_(gz * (fac if ax == -1 else fac[:, None]))
                return gx, None, None

        Scaled.__name__ = Scaled.__qualname__ = cls_name
        return Scaled

    class ShiftDown(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, var, k):
            x = x.detach()
            ctx.var = var
            z = run(call, "shift_down", x, scalar=k, var=var)
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
            return run(call, "evaluate_all_one", x)

        @staticmethod
        @once_differentiable
        def backward(ctx, gz):  # gz broadcast over the item
            return gz[(...,) + (None,) * rank].expand(ctx.shape)

    ns = types.SimpleNamespace(Mul=Mul, Div=Div, Exp=Exp, Log=Log, Pow=Pow, Compose=Compose, Derivative=scaled("Derivative", "derivative"),
                               Coeff=scaled("Coeff", "taylor_expansion_of_coeff"), ShiftDown=ShiftDown, EvalOne=EvalOne)
    _built[(name, rank)] = ns
    return ns
