"""Autograd through genfer_amd.series2_grad (mul, div, exp, log, compose, pow at rank 2) on the MI355X: a grad_fn exactly when one is
due and the forward bits of series2, gradients exact on small integers (against Fractions from the definition),
torch.autograd.gradcheck, the backward passes bit for bit the sequences of public calls documented in the module, and every item
against an independent model -- the six operations as plain torch CPU loops differentiated by torch's own autograd."""
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import REL_TOL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
OPS = ("mul", "div", "exp", "log", "compose0", "compose1", "pow")
BINARY = ("mul", "div", "compose0", "compose1")
E = 3  # pow's exponent where a test takes one


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield


def dense(shape, seed):
    """0.5 + uniform"""
    return 0.5 + np.random.default_rng(seed).random(shape)


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def bits(t):
    return t.detach().contiguous().view(torch.int64)


def host_seed(fn, x):
    """exp / ln of coefficient [0, 0] by the host libm, per item"""
    v = x.detach()[..., 0, 0]
    return torch.tensor([fn(t) for t in v.reshape(-1).tolist()], dtype=torch.float64).reshape(v.shape).to(x.device)


def operands(B, n, nx, second_batch=None):
    """x (compact: nx coefficients) and a full-shape second operand with a dominant constant term (div, log and compose stay tame);
    x has a constant term above 1 as well (it is log's operand)"""
    x = dense((B,) + nx, 100 * n[0] + n[1] + B)
    x[..., 0, 0] += 1.0
    y = dense(((B,) if second_batch is None else second_batch) + n, 200 * n[0] + n[1] + B + 1) / (n[0] * n[1])
    y[..., 0, 0] += 2.0
    return x, y


def call(mod, op, x, y, n, seeded=True, e=E):
    if op == "mul":
        return mod.mul(x, y, n)
    if op == "div":
        return mod.div(x, y, n)
    if op == "exp":
        return mod.exp(x, n, seed=host_seed(math.exp, x) if seeded else None)
    if op == "log":
        return mod.log(x, n, seed=host_seed(math.log, x) if seeded else None)
    if op.startswith("compose"):
        return mod.compose(x, y, int(op[-1]), n)
    return mod.pow(x, e, n)


# ---- propagation ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("op", OPS)
def test_a_result_of_a_tracked_operand_has_a_grad_fn(op):
    from genfer_amd import series2, series2_grad
    from genfer_amd.taylor import TaylorError

    n = (5, 6)
    xa, ya = operands(3, n, (4, 5))
    raw = call(series2, op, dev(xa), dev(ya), n)
    plain = call(series2_grad, op, dev(xa), dev(ya), n)  # nothing tracked: series2's path
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(bits(plain), bits(raw))
    x, y = dev(xa, True), dev(ya)
    z = call(series2_grad, op, x, y, n)
    assert z.grad_fn is not None and z.requires_grad
    assert torch.equal(bits(z), bits(raw))  # the same forward bits on either path
    with torch.no_grad():
        zn = call(series2_grad, op, x, y, n)
    assert zn.grad_fn is None and torch.equal(bits(zn), bits(raw))
    if op in BINARY:  # the second operand alone
        z2 = call(series2_grad, op, dev(xa), dev(ya, True), n)
        assert z2.grad_fn is not None and torch.equal(bits(z2), bits(raw))
    out = torch.empty((3,) + n, dtype=torch.float64, device=DEV)
    fn = getattr(series2_grad, op.rstrip("01"))
    args = (x, y, int(op[-1]), n) if op.startswith("compose") else (x, y, n) if op in BINARY else (x, E, n) if op == "pow" else (x, n)
    with pytest.raises(TaylorError, match="out="):
        fn(*args, out=out)
    with torch.no_grad():  # out= is series2's path when nothing is recorded
        assert fn(*args, out=out) is out
    if op in ("exp", "log"):
        assert torch.equal(bits(out), bits(call(series2, op, dev(xa), None, n, seeded=False)))
        seed = host_seed(getattr(math, op), x).requires_grad_()
        with pytest.raises(TaylorError, match="seed requires grad"):
            fn(x, seed=seed)
        with pytest.raises(TaylorError, match="seed requires grad"):
            fn(x.detach(), seed=seed)
    else:
        assert torch.equal(bits(out), bits(raw))
    with pytest.raises(TaylorError, match="no autograd"):  # the raw layer still refuses
        call(series2, op, x, y, n)


# ---- exact on small integers -------------------------------------------------------------------------------------------------------


def fr_mul(a, b, n):
    out = [[Fraction(0)] * n[1] for _ in range(n[0])]
    for i0, ra in enumerate(a):
        for i1, u in enumerate(ra):
            for j0, rb in enumerate(b):
                for j1, v in enumerate(rb):
                    if i0 + j0 < n[0] and i1 + j1 < n[1]:
                        out[i0 + j0][i1 + j1] += u * v
    return out


def fr_unit(n):
    out = [[Fraction(0)] * n[1] for _ in range(n[0])]
    out[0][0] = Fraction(1)
    return out


def fr_inv(y, n):
    """1 / y for y[0][0] == 1: the geometric series sum_k (1 - y)^k, which ends by degree"""
    d = [[(1 if (i, j) == (0, 0) else 0) - (y[i][j] if i < len(y) and j < len(y[0]) else 0) for j in range(n[1])] for i in range(n[0])]
    assert d[0][0] == 0
    r, p = fr_unit(n), fr_unit(n)
    for _ in range(n[0] + n[1]):
        p = fr_mul(p, d, n)
        r = [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(r, p)]
    return r


def fr_pow(x, e, n):
    r = fr_unit(n)
    for _ in range(e):
        r = fr_mul(r, x, n)
    return r


def fr_scale(a, c):
    return [[c * v for v in row] for row in a]


def fr_vjp(gz, kernel, m):
    """sum_k gz[k] * kernel[k - j] for j < m: the gradient where dz_k / dx_j = kernel[k - j]"""
    n = (len(gz), len(gz[0]))
    return [[sum(gz[k0][k1] * kernel[k0 - j0][k1 - j1] for k0 in range(j0, n[0]) for k1 in range(j1, n[1])) for j1 in range(m[1])] for j0 in range(m[0])]


def fr_dot(a, b):
    return sum(u * v for ra, rb in zip(a, b) for u, v in zip(ra, rb))


def ints(shape, seed, lo=-2, hi=2):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float64)


def fr(item):
    return [[Fraction(int(v)) for v in row] for row in item]


def floats(rows):
    return [[float(v) for v in r] for r in rows]


def test_exact_gradients_on_small_integers():
    from genfer_amd import series2_grad as sg

    B, n, nx = 2, (3, 4), (2, 3)
    xa, ya, ga = ints((B,) + nx, 1), ints((B,) + n, 2), ints((B,) + n, 3)
    ya[:, 0, 0] = 1.0  # a divisor with integer quotients
    gz = dev(ga)

    def grads(fn, *ops):
        ts = [dev(o, True) for o in ops]
        fn(*ts).backward(gz)
        return [t.grad.cpu().numpy() for t in ts]

    # mul: dz_k / dx_j = y_{k-j}
    gx, gy = grads(lambda x, y: sg.mul(x, y, n), xa, ya)
    for b in range(B):
        assert gx[b].tolist() == floats(fr_vjp(fr(ga[b]), fr(ya[b]), nx)), b
        assert gy[b].tolist() == floats(fr_vjp(fr(ga[b]), fr_mul(fr(xa[b]), fr_unit(n), n), n)), b
    # div: dr_k / dx_j = (1 / y)_{k-j}, dr_k / dy_j = -(r / y)_{k-j}
    gx, gy = grads(lambda x, y: sg.div(x, y, n), xa, ya)
    for b in range(B):
        iy = fr_inv(fr(ya[b]), n)
        r = fr_mul(fr(xa[b]), iy, n)
        assert gx[b].tolist() == floats(fr_vjp(fr(ga[b]), iy, nx)), b
        assert gy[b].tolist() == floats(fr_scale(fr_vjp(fr(ga[b]), fr_mul(r, iy, n), n), -1)), b
    # log of an operand with x[0][0] == 1: dl_k / dx_j = (1 / x)_{k-j}
    xl = xa.copy()
    xl[:, 0, 0] = 1.0
    (gx,) = grads(lambda x: sg.log(x, n), xl)
    for b in range(B):
        assert gx[b].tolist() == floats(fr_vjp(fr(ga[b]), fr_inv(fr(xl[b]), n), nx)), b
    # exp of an operand with x[0][0] == 0 (the seed is 1) and coefficients that are multiples of 60: de_k / dx_j = e_{k-j}, and
    # e = sum_k x^k / k! has integer coefficients (x^k ends at total degree 5 here and 60^k / k! is an integer for k <= 5), so the
    # forward recurrence and the gradient are exact
    xe = 60.0 * ints((B,) + nx, 4, -1, 1)
    xe[:, 0, 0] = 0.0
    (gx,) = grads(lambda x: sg.exp(x, n, seed=torch.ones(B, dtype=torch.float64, device=DEV)), xe)
    for b in range(B):
        ex, p = fr_unit(n), fr_unit(n)
        for k in range(1, n[0] + n[1]):
            p = fr_scale(fr_mul(p, fr(xe[b]), n), Fraction(1, k))
            ex = [[u + v for u, v in zip(ra, rb)] for ra, rb in zip(ex, p)]
        assert all(v.denominator == 1 for row in ex for v in row)
        assert gx[b].tolist() == floats(fr_vjp(fr(ga[b]), ex, nx)), b
    # pow: dp_k / dx_j = e * (x^(e-1))_{k-j}
    for e in (0, 1, 3):
        (gx,) = grads(lambda x: sg.pow(x, e, n), xa)
        for b in range(B):
            kern = fr_scale(fr_pow(fr(xa[b]), e - 1, n), e) if e > 0 else fr_scale(fr_unit(n), 0)
            assert gx[b].tolist() == floats(fr_vjp(fr(ga[b]), kern, nx)), (e, b)
    # compose: dh / df[slice i] = g^i (along the axis that stays), dh_k / dg_j = (df / dvar)(g)_{k-j}
    for var in (0, 1):
        gf, gg = grads(lambda f, g: sg.compose(f, g, var, n), xa, ya)
        for b in range(B):
            f, g, gb = fr(xa[b]), fr(ya[b]), fr(ga[b])
            S = nx[var]
            fp = fr_scale(fr_unit(n), 0)
            for i in range(S):
                gi = fr_pow(g, i, n)
                for c in range(nx[1 - var]):
                    # the monomial of the axis that stays, t^c, times g^i: a shift of g^i by c along that axis
                    mono = [[Fraction(0)] * (c + 1) for _ in range(1)] if var == 0 else [[Fraction(0)] for _ in range(c + 1)]
                    mono[-1][-1] = Fraction(1)
                    want = fr_dot(gb, fr_mul(gi, mono, n))
                    got = gf[b][i][c] if var == 0 else gf[b][c][i]
                    assert float(want) == got, (var, b, i, c)
                    if i >= 1:
                        coef = f[i][c] if var == 0 else f[c][i]
                        term = fr_scale(fr_mul(fr_pow(g, i - 1, n), mono, n), i * coef)
                        fp = [[u + v for u, v in zip(ra, rb)] for ra, rb in zip(fp, term)]
            assert gg[b].tolist() == floats(fr_vjp(gb, fp, n)), (var, b)


# ---- finite differences ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("op", ["mul", "div", "exp", "log", "exp_device_seed", "log_device_seed", "compose0", "compose1", "pow"])
def test_gradcheck(op):
    from genfer_amd import series2_grad

    B, n, nx = 2, (3, 4), (2, 3)
    xa, ya = operands(B, n, nx)
    x, y = dev(xa, True), dev(ya, True)
    base = op.split("_")[0]
    if base in BINARY:
        assert torch.autograd.gradcheck(lambda a, b: call(series2_grad, base, a, b, n), (x, y))
    else:
        assert torch.autograd.gradcheck(lambda a: call(series2_grad, base, a, None, n, seeded=not op.endswith("device_seed")), (x,))


# ---- the documented sequences, bit for bit -----------------------------------------------------------------------------------------


def sequence(op, x, y, gz, n, result):
    """the module docstring of series2_grad with explicit public calls on detached tensors: (gx, gy)"""
    from genfer_amd import series2

    one = torch.ones((1, 1), dtype=torch.float64, device=DEV)
    nx = tuple(x.shape[-2:])
    if op == "mul":
        return series2.corr(gz, y, nx), series2.corr(gz, x, y.shape[-2:])
    if op == "div":
        u = series2.corr(gz, series2.div(one, y, n), n)
        return u[..., :nx[0], :nx[1]], -series2.corr(u, result, y.shape[-2:])
    if op == "exp":
        return series2.corr(gz, result, nx), None
    if op == "log":
        return series2.corr(gz, series2.div(one, x, n), nx), None
    if op == "pow":
        return E * series2.corr(gz, series2.pow(x, E - 1, n), nx), None
    var = int(op[-1])
    i = torch.arange(1, nx[var], dtype=torch.float64, device=DEV)
    fp = x[..., 1:, :] * i[:, None] if var == 0 else x[..., :, 1:] * i
    return series2._compose_adj(gz, y, var, nx), series2.corr(gz, series2.compose(fp, y, var, n), y.shape[-2:])


@pytest.mark.parametrize("B,n", [(3, (4, 5)), (2, (12, 11))])
@pytest.mark.parametrize("op", OPS)
def test_backward_is_the_documented_sequence(op, B, n):
    from genfer_amd import series2_grad

    nx = (n[0] - 1, n[1] - 1)
    xa, ya = operands(B, n, nx)
    ga = dense((B,) + n, 7 * n[0] + B) - 1.0
    x, y, gz = dev(xa, True), dev(ya, op in BINARY), dev(ga)
    z = call(series2_grad, op, x, y, n)
    z.backward(gz)
    with torch.no_grad():
        gx, gy = sequence(op, x.detach(), y.detach(), gz, n, z.detach())
    assert torch.equal(bits(x.grad), bits(gx)), op
    if op in BINARY:
        assert torch.equal(bits(y.grad), bits(gy)), op
    else:
        assert y.grad is None


def test_backward_with_one_slice_and_zero_exponent():
    from genfer_amd import series2, series2_grad

    n = (3, 4)
    ga = dense((2,) + n, 5)
    for var, fs in ((0, (1, 3)), (1, (3, 1))):
        fa, ya = operands(2, n, fs)
        f, g = dev(fa, True), dev(ya, True)
        series2_grad.compose(f, g, var, n).backward(dev(ga))
        assert torch.equal(bits(f.grad), bits(dev(ga)[..., :fs[0], :fs[1]]))
        want = series2.corr(dev(ga), series2.compose(torch.zeros_like(f.detach()), g.detach(), var, n), n)
        assert torch.equal(bits(g.grad), bits(want)) and not bool(g.grad.any())
    x = dev(operands(2, n, (2, 3))[0], True)
    series2_grad.pow(x, 0, n).backward(dev(ga))
    assert x.grad.shape == x.shape and not bool(x.grad.any())


# ---- against an independent model --------------------------------------------------------------------------------------------------
# the six operations as plain loops over torch CPU float64 tensors, differentiated by torch itself.  A series is a dict-free dense
# tensor [..., n0, n1]; the product is written over the rows of the first factor with shifts, nothing shared with the library.


def m_mul(x, y, n):
    batch = torch.broadcast_shapes(x.shape[:-2], y.shape[:-2])
    out = torch.zeros(batch + n, dtype=torch.float64)
    for i0 in range(min(x.shape[-2], n[0])):
        for i1 in range(min(x.shape[-1], n[1])):
            r0, r1 = min(y.shape[-2], n[0] - i0), min(y.shape[-1], n[1] - i1)
            pad = torch.nn.functional.pad(x[..., i0:i0 + 1, i1:i1 + 1] * y[..., :r0, :r1], (i1, n[1] - i1 - r1, i0, n[0] - i0 - r0))
            out = out + pad
    return out


def m_inv(y, n):
    """1 / y by Newton-free recursion on total degree: r = (1 - (y - y00) * r) / y00, iterated until the truncation is exact"""
    y00 = y[..., :1, :1]
    rest = torch.nn.functional.pad(y, (0, n[1] - y.shape[-1], 0, n[0] - y.shape[-2])).clone()
    mask = torch.ones(n, dtype=torch.float64)
    mask[0, 0] = 0.0
    rest = rest * mask
    unit = torch.zeros(n, dtype=torch.float64)
    unit[0, 0] = 1.0
    r = unit / y00
    for _ in range(n[0] + n[1]):
        r = (unit - m_mul(rest, r, n)) / y00
    return r


def m_exp(x, n):
    """exp(x00) * sum_k (x - x00)^k / k!, which ends by degree"""
    mask = torch.ones(x.shape[-2:], dtype=torch.float64)
    mask[0, 0] = 0.0
    d = x * mask
    term = torch.zeros(x.shape[:-2] + n, dtype=torch.float64)
    term[..., 0, 0] = 1.0
    total = term
    for k in range(1, n[0] + n[1]):
        term = m_mul(term, d, n) / k
        total = total + term
    return total * torch.exp(x[..., :1, :1])


def m_log(x, n):
    """ln(x00) + sum_k (-1)^(k+1) u^k / k, u = (x - x00) / x00"""
    mask = torch.ones(x.shape[-2:], dtype=torch.float64)
    mask[0, 0] = 0.0
    u = x * mask / x[..., :1, :1]
    p = torch.zeros(x.shape[:-2] + n, dtype=torch.float64)
    p[..., 0, 0] = 1.0
    total = torch.zeros(x.shape[:-2] + n, dtype=torch.float64)
    for k in range(1, n[0] + n[1]):
        p = m_mul(p, u, n)
        total = total + p * ((-1.0) ** (k + 1) / k)
    const = torch.zeros(n, dtype=torch.float64)
    const[0, 0] = 1.0
    return total + const * torch.log(x[..., :1, :1])


def m_compose(f, g, var, n):
    """sum_i slice_i(f) * g^i, the slice a series in the variable that stays"""
    batch = torch.broadcast_shapes(f.shape[:-2], g.shape[:-2])
    total = torch.zeros(batch + n, dtype=torch.float64)
    p = torch.zeros(n, dtype=torch.float64)
    p[0, 0] = 1.0
    for i in range(f.shape[var - 2]):
        sl = f[..., i:i + 1, :] if var == 0 else f[..., :, i:i + 1]
        total = total + m_mul(sl, p, n)
        p = m_mul(p, g, n)
    return total


def m_pow(x, e, n):
    r = torch.zeros(n, dtype=torch.float64)
    r[0, 0] = 1.0
    for _ in range(e):
        r = m_mul(r, x, n)
    return r


def model(op, x, y, n):
    if op == "mul":
        return m_mul(x, y, n)
    if op == "div":
        return m_mul(x, m_inv(y, n), n)
    if op == "exp":
        return m_exp(x, n)
    if op == "log":
        return m_log(x, n)
    if op == "pow":
        return m_pow(x, E, n)
    return m_compose(x, y, int(op[-1]), n)


_model_grads = {}


def model_grads(op, B, n, nx, second_batch):
    """the model's gradients, computed once per case and left unchanged"""
    key = (op, B, n, nx, second_batch)
    if key not in _model_grads:
        xa, ya = operands(B, n, nx, second_batch)
        if op == "log":
            xa = xa / (n[0] * n[1])  # |x - x00| / x00 well inside the radius of the logarithm's series
            xa[..., 0, 0] += 2.0
        if op == "exp":
            xa = xa / 2.0
        ga = dense((B,) + n, 17 * n[0] + B) - 1.0
        xc, yc = torch.from_numpy(xa.copy()).requires_grad_(), torch.from_numpy(ya.copy()).requires_grad_(op in BINARY)
        model(op, xc, yc, n).backward(torch.from_numpy(ga))
        _model_grads[key] = (xa, ya, ga, xc.grad, yc.grad)
    return _model_grads[key]


# (4, 5) with a compact x of (3, 4) and B = 3; (12, 11): more than one wave; a second operand of batch shape (): sum_to_size reduces
MODEL_CASES = [(op, B, n, nx, None) for op in OPS for B, n, nx in ((3, (4, 5), (3, 4)), (2, (12, 11), (12, 11)))]
MODEL_CASES += [(op, 3, (4, 5), (3, 4), ()) for op in BINARY]


@pytest.mark.parametrize("op,B,n,nx,second_batch", MODEL_CASES)
def test_gradients_against_the_model(op, B, n, nx, second_batch):
    from genfer_amd import series2_grad

    xa, ya, ga, want_x, want_y = model_grads(op, B, n, nx, second_batch)
    x, y = dev(xa, True), dev(ya, op in BINARY)
    call(series2_grad, op, x, y, n, seeded=False).backward(dev(ga))  # device seeds: the model's exp / log are torch's
    pairs = [("first", x.grad.cpu(), want_x)] + ([("second", y.grad.cpu(), want_y)] if op in BINARY else [])
    for which, got, want in pairs:
        assert got.shape == want.shape
        scale = want.abs().amax(dim=-1, keepdim=True)  # every row, against its own largest gradient
        err = (got - want).abs()
        worst = float((err / scale).max())
        print(f"{op} B={B} n={n} {which}: worst row error {worst:.3e} of the row's largest gradient")
        assert bool((err <= REL_TOL * scale).all()), (op, B, n, which, worst)


# ---- other cases -------------------------------------------------------------------------------------------------------------------


def test_expanded_grad_output():
    """z.sum().backward() hands over an expanded scalar (stride 0 on the series axes): it is made contiguous first"""
    from genfer_amd import series2_grad

    n = (4, 5)
    xa, ya = operands(3, n, (3, 4))
    x, y = dev(xa, True), dev(ya, True)
    series2_grad.mul(x, y, n).sum().backward()
    x2, y2 = dev(xa, True), dev(ya, True)
    series2_grad.mul(x2, y2, n).backward(torch.ones((3,) + n, dtype=torch.float64, device=DEV))
    assert torch.equal(bits(x.grad), bits(x2.grad)) and torch.equal(bits(y.grad), bits(y2.grad))


def test_only_the_needed_gradient_is_computed(monkeypatch):
    from genfer_amd import series2, series2_grad

    n = (4, 5)
    fa, ga = operands(3, n, (3, 4))
    gz = torch.ones((3,) + n, dtype=torch.float64, device=DEV)
    f, g = dev(fa, True), dev(ga)
    calls = []
    real_corr, real_adj = series2.corr, series2._compose_adj
    monkeypatch.setattr(series2, "corr", lambda *a, **k: (calls.append("corr"), real_corr(*a, **k))[1])
    monkeypatch.setattr(series2, "_compose_adj", lambda *a, **k: (calls.append("adj"), real_adj(*a, **k))[1])
    series2_grad.compose(f, g, 1, n).backward(gz)
    assert calls == ["adj"] and g.grad is None
    calls.clear()
    f2, g2 = dev(fa), dev(ga, True)
    series2_grad.compose(f2, g2, 1, n).backward(gz)
    assert calls == ["corr"] and f2.grad is None and g2.grad is not None
    calls.clear()
    x, y = dev(fa, True), dev(ga)
    series2_grad.mul(x, y, n).backward(gz)
    assert calls == ["corr"] and y.grad is None
