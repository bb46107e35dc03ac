"""The transposed bivariate operations (genfer_amd.series2.corr / _compose_adj, gft_series2_corr / gft_series2_compose_adj) and the
differentiable module genfer_amd.series2_grad without a GPU: the numpy model of tests/_series2_adj_model.py against the existing
product model on flipped arrays (the GPU tests use it as their integer oracle), the exported surface, and every refusal that the
Python side makes before it touches a device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _series2_adj_model as A
import _series2_model as M
from conftest import ROOT

SYMBOLS = ("gft_series2_corr", "gft_series2_compose_adj")
OPS = ("mul", "div", "exp", "log", "compose", "pow")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def mixed(shape, seed):
    """mixed signs with some exact zeros"""
    rng = np.random.default_rng(seed)
    a = rng.random(shape) - 0.5
    a[rng.random(shape) < 0.15] = 0.0
    return a


def flip(a):
    return np.ascontiguousarray(a[..., ::-1, ::-1])


# ---- the model -------------------------------------------------------------------------------------------------------------------

CORR_CASES = [  # g, y, m
    ((1, 1), (1, 1), (1, 1)), ((1, 7), (1, 7), (1, 7)), ((7, 1), (3, 1), (7, 1)), ((3, 5), (3, 5), (3, 5)), ((3, 5), (1, 5), (3, 5)),
    ((3, 5), (3, 1), (2, 5)), ((3, 5), (2, 3), (3, 4)), ((6, 4), (5, 2), (1, 1)), ((9, 5), (4, 5), (9, 2)),
]


@pytest.mark.parametrize("g,y,m", CORR_CASES)
def test_corr_model_is_the_flipped_product(g, y, m):
    """corr2(g, y)[i0][i1] is bit for bit mul2(flip(g), y, g.shape)[g0-1-i0][g1-1-i1]"""
    ga, ya = mixed(g, 3 * g[0] + g[1]), mixed(y, 5 * y[0] + y[1])
    want = flip(M.mul(flip(ga), ya, g))[:m[0], :m[1]]
    assert same_bits(A.corr2(ga, ya, m), want)


def test_corr_model_forms_no_term_from_padding():
    """a compact y beside an infinity in g: a padded zero would turn the outputs it does not reach into NaN"""
    g = np.array([[1.0, 2.0, 3.0], [4.0, np.inf, 6.0]])
    c = A.corr2(g, np.array([[2.0, 1.0]]), (2, 3))
    assert same_bits(c, np.array([[4.0, 7.0, 6.0], [np.inf, np.inf, 12.0]]))
    assert same_bits(c, flip(M.mul(flip(g), np.array([[2.0, 1.0]]), (2, 3))))


def test_adjoint_identity_in_integers():
    """<mul(x, y, n), g> = <x, corr(g, y, x.shape)> exactly on small integers, compact operands included"""
    rng = np.random.default_rng(5)
    for nx, ny, n in [((3, 4), (3, 4), (3, 4)), ((2, 3), (3, 4), (3, 4)), ((3, 4), (1, 2), (3, 4)), ((1, 1), (1, 1), (1, 1)), ((2, 2), (2, 3), (4, 5))]:
        x, y, g = (rng.integers(-3, 4, size=s).astype(np.float64) for s in (nx, ny, n))
        assert float((M.mul(x, y, n) * g).sum()) == float((x * A.corr2(g, y, nx)).sum())


def fwd_compose(f, g, var, n):
    """the forward Horner loop of gft_series2_compose on the existing product model"""
    S = f.shape[var]
    sl = lambda i: (f[i:i + 1, :] if var == 0 else f[:, i:i + 1])  # noqa: E731
    res = 0.0 + sl(S - 1)
    for i in range(S - 2, -1, -1):
        L = tuple(min(res.shape[a] + g.shape[a] - 1, n[a]) for a in (0, 1))
        res = M.mul(res, g, L)
        if var == 0:
            res[0, :f.shape[1]] += f[i]
        else:
            res[:f.shape[0], 0] += f[:, i]
    out = np.zeros(n)
    out[:res.shape[0], :res.shape[1]] = res
    return out


ADJ_CASES = [  # f, g, n
    ((5, 3), (2, 3), (6, 7)), ((1, 4), (2, 3), (3, 4)), ((4, 1), (2, 3), (4, 3)), ((3, 2), (1, 3), (3, 4)), ((2, 3), (3, 1), (3, 4)), ((2, 3), (3, 4), (3, 4)),
]


@pytest.mark.parametrize("var", [0, 1])
@pytest.mark.parametrize("f,g,n", ADJ_CASES)
def test_compose_adj_model_is_the_adjoint_of_compose_in_f(f, g, n, var):
    """<compose(f, g), gh> = <f, compose_adj(gh, g)> exactly on small integers: compose is linear in f"""
    rng = np.random.default_rng(7 * f[0] + f[1] + var)
    fa, ga, gh = (rng.integers(-2, 3, size=s).astype(np.float64) for s in (f, g, n))
    L = A.compact_shapes(f, g, n, var)
    assert L[-1] == ((1, f[1]) if var == 0 else (f[0], 1)) and all(L[i][a] >= L[i + 1][a] for i in range(len(L) - 1) for a in (0, 1))
    adj = A.compose_adj(gh, ga, var, f)
    assert adj.shape == f
    assert float((fwd_compose(fa, ga, var, n) * gh).sum()) == float((fa * adj).sum())


def test_compose_adj_model_with_one_slice_is_the_leading_entries():
    gh = mixed((3, 4), 1)
    g = np.full((2, 2), np.nan)  # not read
    assert same_bits(A.compose_adj(gh, g, 0, (1, 4)), gh[:1, :4])
    assert same_bits(A.compose_adj(gh, g, 1, (3, 1)), gh[:3, :1])


# ---- the surface -----------------------------------------------------------------------------------------------------------------


def test_symbols_are_declared_and_exported():
    import genfer_amd

    if not os.path.exists(genfer_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    L = genfer_amd.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert hasattr(L, s), s
        assert f"pub fn {s}(" in doc, s
    assert not hasattr(L, "gfti_series2_corr") and not hasattr(L, "gfti_series2_compose_adj")  # no interval twins


def test_module_is_re_exported():
    import genfer_amd
    from genfer_amd import series2, series2_grad

    assert genfer_amd.series2_grad is series2_grad
    for f in OPS:
        assert callable(getattr(series2_grad, f))
    assert callable(series2.corr) and callable(series2._compose_adj)
    assert "series2_grad" in series2.__doc__
    for word in ("corr(gz, y, x.shape[-2:])", "u = corr(gr, div(one, y, n), n)", "corr(ge, e, x.shape[-2:])", "corr(gl, div(one, x, n), x.shape[-2:])",
                 "e * corr(gp, pow(x, e - 1, n), x.shape[-2:])", "_compose_adj(gh, g, var, f.shape[-2:])", "corr(gh, compose(fp, g, var, n), g.shape[-2:])"):
        assert word in series2_grad.__doc__, word  # the documented sequences


def test_series2_grad_imports_without_torch():
    code = "import sys; sys.modules['torch'] = None\nfrom genfer_amd import series2_grad, series2\nassert callable(series2_grad.mul)\nprint('ok')"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_bench_series2_grad_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_series2_grad.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "--ops" in out.stdout and "--corr-shapes" in out.stdout and "--rounds" in out.stdout


# ---- refusals that need no device ------------------------------------------------------------------------------------------------


def test_corr_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    from genfer_amd import series2
    from genfer_amd.taylor import TaylorError

    g = torch.ones((3, 4, 8), dtype=torch.float64)
    y = torch.ones((3, 2, 5), dtype=torch.float64)
    with pytest.raises(TaylorError, match="short side"):
        series2.corr(g, y, m=(5, 8))  # m exceeds g
    with pytest.raises(TaylorError, match="short side"):
        series2.corr(g, y, m=(4, 9))
    with pytest.raises(TaylorError, match="more than the 4 of g"):
        series2.corr(g, torch.ones((3, 5, 5), dtype=torch.float64))  # y exceeds g
    with pytest.raises(TaylorError, match="more than the 8 of g"):
        series2.corr(g, torch.ones((3, 2, 9), dtype=torch.float64))
    with pytest.raises(TaylorError, match="is empty"):
        series2.corr(g[:, :0], y)
    with pytest.raises(TaylorError, match="is empty"):
        series2.corr(g, y[:, :, :0])
    with pytest.raises(TaylorError, match="at least one coefficient"):
        series2.corr(g, y, m=(0, 8))
    with pytest.raises(TaylorError, match="unit stride"):
        series2.corr(g[:, :, ::2], y[:, :, :4])
    with pytest.raises(TaylorError, match="unit stride"):
        series2.corr(g, y[:, :, ::2])
    big = torch.ones((17, 241), dtype=torch.float64)  # 4097
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series2.corr(big, y[0])
    with pytest.raises(TaylorError, match="float32"):
        series2.corr(g.float(), y)
    with pytest.raises(TaylorError, match="float32"):
        series2.corr(g, y.float())
    with pytest.raises(TaylorError, match="at least 2"):
        series2.corr(g[0, 0], y)
    with pytest.raises(TypeError, match="pair"):
        series2.corr(g, y, m=8)
    with pytest.raises(TypeError, match="torch.Tensor"):
        series2.corr([[1.0]], y)
    with pytest.raises(TaylorError, match=r"out has \(4, 8\)"):
        series2.corr(g, y, m=(2, 5), out=torch.empty((3, 4, 8), dtype=torch.float64))
    with pytest.raises(TaylorError, match="no autograd"):
        series2.corr(g.clone().requires_grad_(), y)
    with pytest.raises(TaylorError, match="on cpu"):  # everything else in order: the placement is judged last
        series2.corr(g, y, m=(2, 5))
    meta = torch.zeros((3, 4, 8), dtype=torch.float64, device="meta")
    with pytest.raises(TaylorError, match="on meta"):
        series2.corr(meta, meta)


def test_compose_adj_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    from genfer_amd import series2
    from genfer_amd.taylor import TaylorError

    gh = torch.ones((3, 4, 8), dtype=torch.float64)
    g = torch.ones((3, 2, 5), dtype=torch.float64)
    for var in (2, -1, True, 0.0, None):
        with pytest.raises(TaylorError, match="is 0 or 1"):
            series2._compose_adj(gh, g, var, (2, 3))
    with pytest.raises(TaylorError, match="short side"):
        series2._compose_adj(gh, g, 0, (5, 3))  # nf exceeds n
    with pytest.raises(TaylorError, match="short side"):
        series2._compose_adj(gh, g, 1, (2, 9))
    with pytest.raises(TaylorError, match="more than the 4 of gh"):
        series2._compose_adj(gh, torch.ones((5, 5), dtype=torch.float64), 0, (2, 3))  # g exceeds n
    with pytest.raises(TaylorError, match="is empty"):
        series2._compose_adj(gh[:, :, :0], g, 0, (2, 3))
    with pytest.raises(TaylorError, match="at least one coefficient"):
        series2._compose_adj(gh, g, 0, (2, 0))
    with pytest.raises(TaylorError, match="unit stride"):
        series2._compose_adj(gh[:, :, ::2], g[:, :, :4], 0, (2, 3))
    with pytest.raises(TaylorError, match="exceeds the limit of 4096"):
        series2._compose_adj(torch.ones((17, 241), dtype=torch.float64), g[0], 0, (2, 3))
    with pytest.raises(TaylorError, match="float32"):
        series2._compose_adj(gh.float(), g, 0, (2, 3))
    with pytest.raises(TaylorError, match="on cpu"):  # the placement is judged last
        series2._compose_adj(gh, g, 0, (2, 3))


@pytest.mark.parametrize("op", OPS)
def test_series2_grad_refusals_need_no_device(op):
    torch = pytest.importorskip("torch")
    from genfer_amd import series2, series2_grad
    from genfer_amd.taylor import TaylorError

    x = torch.ones((3, 4, 8), dtype=torch.float64)
    xg = x.clone().requires_grad_()
    out = torch.empty((3, 4, 8), dtype=torch.float64)
    args = {"mul": (xg, x), "div": (x, xg), "compose": (xg, x), "pow": (xg, 3)}.get(op, (xg,))
    with pytest.raises(TaylorError, match=r"out= cannot be combined with an operand that requires grad"):
        getattr(series2_grad, op)(*args, out=out)
    if op in ("exp", "log"):
        seed = torch.ones(3, dtype=torch.float64, requires_grad=True)
        for operand in (xg, x):
            with pytest.raises(TaylorError, match="seed requires grad"):
                getattr(series2_grad, op)(operand, seed=seed)
    if op == "compose":
        with pytest.raises(TaylorError, match="is 0 or 1"):
            series2_grad.compose(xg, x, var=2)
    if op == "pow":
        with pytest.raises(TaylorError, match="negative"):
            series2_grad.pow(xg, -1)
    # the raw layer keeps its refusal, with its wording; the differentiable twin goes on to the placement
    with pytest.raises(TaylorError, match="this version of series2 has no autograd"):
        getattr(series2, op)(*args)
    with pytest.raises(TaylorError, match="on cpu"):
        getattr(series2_grad, op)(*args)
    with torch.no_grad():  # grad mode off: series2's path, out= allowed (and then refused for where it lives)
        with pytest.raises(TaylorError, match=f"series2.{op}: .* on cpu"):
            getattr(series2_grad, op)(*args, out=out)


def test_series2_mul_still_refuses_a_tracked_operand():
    torch = pytest.importorskip("torch")
    from genfer_amd import series2
    from genfer_amd.taylor import TaylorError

    x = torch.ones((2, 3), dtype=torch.float64)
    with pytest.raises(TaylorError, match="no autograd"):
        series2.mul(x.clone().requires_grad_(), x)
    with pytest.raises(TaylorError, match="no autograd"):
        series2.mul(x, x.clone().requires_grad_())
