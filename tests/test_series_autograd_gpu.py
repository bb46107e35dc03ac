"""Autograd through genfer_amd.series (mul, div, exp, log, compose, pow) on the MI355X: a grad_fn where one is due and forward bits
unchanged, gradients exact on small integers (against Fractions from the definition), torch.autograd.gradcheck in both forms, the
backward passes bit for bit the documented sequences of public calls, and every row against an independent model -- the six
operations as plain torch CPU loops differentiated by torch's own autograd."""
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import REL_TOL
from test_series_compose_cpu import dense

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
OPS = ("mul", "div", "exp", "log", "compose", "pow")


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield
    genfer_amd.series.set_form(None)


@pytest.fixture(autouse=True)
def _auto_form():
    from genfer_amd import series

    series.set_form(None)
    yield
    series.set_form(None)


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def bits(t):
    return t.detach().contiguous().view(torch.int64)


def host_seed(fn, x):
    """exp / ln of coefficient 0 by the host libm, per item"""
    v = x.detach()[..., 0]
    return torch.tensor([fn(t) for t in v.reshape(-1).tolist()], dtype=torch.float64).reshape(v.shape).to(x.device)


def operands(B, n, nx, second_shape=None):
    """x (nx coefficients a row) and a full-length second operand with a dominant constant term (div, log and compose stay tame)"""
    x = dense((B, nx), 100 * n + B)
    y = dense(second_shape or (B, n), 200 * n + B + 1) / n
    y[..., 0] += 2.0
    return x, y


def call(op, x, y, n, seeded=True):
    from genfer_amd import series

    if op == "mul":
        return series.mul(x, y, n)
    if op == "div":
        return series.div(x, y, n)
    if op == "exp":
        return series.exp(x, n, seed=host_seed(math.exp, x) if seeded else None)
    if op == "log":
        return series.log(x, n, seed=host_seed(math.log, x) if seeded else None)
    if op == "compose":
        return series.compose(x, y, n)
    return series.pow(x, 5, n)


BINARY = ("mul", "div", "compose")

# ---- propagation ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("op", OPS)
def test_a_result_of_a_tracked_operand_has_a_grad_fn(op):
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    xa, ya = operands(5, 12, 9)
    xa[:, 0] += 1.0
    plain = call(op, dev(xa), dev(ya), 12)
    assert plain.grad_fn is None and not plain.requires_grad
    x, y = dev(xa, True), dev(ya)
    z = call(op, x, y, 12)
    assert z.grad_fn is not None and z.requires_grad
    assert torch.equal(bits(z), bits(plain))  # the same forward bits on either path
    with torch.no_grad():
        zn = call(op, x, y, 12)
    assert zn.grad_fn is None and torch.equal(bits(zn), bits(plain))
    if op in BINARY:  # the second operand alone
        z2 = call(op, dev(xa), dev(ya, True), 12)
        assert z2.grad_fn is not None and torch.equal(bits(z2), bits(plain))
    out = torch.empty((5, 12), dtype=torch.float64, device=DEV)
    args = (x, y, 12) if op in BINARY else (x, 5, 12) if op == "pow" else (x, 12)
    with pytest.raises(TaylorError, match="out="):
        getattr(series, op)(*args, out=out)
    with torch.no_grad():  # out= is today's path when nothing is recorded
        getattr(series, op)(*args, out=out)
    if op in ("exp", "log"):
        seed = host_seed(getattr(math, op), x).requires_grad_()
        with pytest.raises(TaylorError, match="seed requires grad"):
            getattr(series, op)(x, seed=seed)
        with pytest.raises(TaylorError, match="seed requires grad"):
            getattr(series, op)(x.detach(), seed=seed)


# ---- exact on small integers -------------------------------------------------------------------------------------------------------


def fr_mul(a, b, n):
    out = [Fraction(0)] * n
    for i, u in enumerate(a):
        for j, v in enumerate(b):
            if i + j < n:
                out[i + j] += u * v
    return out


def fr_inv(y, n):
    r = [Fraction(0)] * n
    for k in range(n):
        s = Fraction(1 if k == 0 else 0) - sum(r[j] * y[k - j] for j in range(k) if k - j < len(y))
        r[k] = s / y[0]
    return r


def fr_pow(x, e, n):
    r = [Fraction(1)] + [Fraction(0)] * (n - 1)
    for _ in range(e):
        r = fr_mul(r, x, n)
    return r


def fr_vjp(gz, kernel, m):
    """sum_k gz[k] * kernel[k - j] for j < m: the gradient where dz_k / dx_j = kernel[k - j]"""
    return [sum(gz[k] * kernel[k - j] for k in range(j, len(gz))) for j in range(m)]


def ints(shape, seed, lo=-3, hi=3):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float64)


def fr(row):
    return [Fraction(int(v)) for v in row]


def as_floats(rows):
    return np.array([[float(v) for v in r] for r in rows])


def test_exact_gradients_on_small_integers():
    from genfer_amd import series

    B, n, nx = 3, 6, 4
    xa, ya, ga = ints((B, nx), 1), ints((B, n), 2), ints((B, n), 3)
    ya[:, 0] = 1.0  # a divisor with integer quotients
    gz = dev(ga)

    def grads(fn, *ops):
        ts = [dev(o, True) for o in ops]
        fn(*ts).backward(gz)
        return [t.grad.cpu().numpy() for t in ts]

    # mul: dz_k / dx_j = y_{k-j}
    gx, gy = grads(lambda x, y: series.mul(x, y, n), xa, ya)
    assert np.array_equal(gx, as_floats([fr_vjp(fr(ga[b]), fr(ya[b]), nx) for b in range(B)]))
    assert np.array_equal(gy, as_floats([fr_vjp(fr(ga[b]), fr(xa[b]) + [Fraction(0)] * (n - nx), n) for b in range(B)]))
    # div: dr_k / dx_j = (1 / y)_{k-j}, dr_k / dy_j = -(r / y)_{k-j}
    gx, gy = grads(lambda x, y: series.div(x, y, n), xa, ya)
    for b in range(B):
        iy = fr_inv(fr(ya[b]), n)
        r = fr_mul(fr(xa[b]), iy, n)
        assert gx[b].tolist() == [float(v) for v in fr_vjp(fr(ga[b]), iy, nx)], b
        assert gy[b].tolist() == [float(-v) for v in fr_vjp(fr(ga[b]), fr_mul(r, iy, n), n)], b
    # pow: dp_k / dx_j = e * (x^(e-1))_{k-j}
    for e in (0, 1, 2, 5):
        (gx,) = grads(lambda x: series.pow(x, e, n), xa)
        for b in range(B):
            kern = [e * v for v in fr_pow(fr(xa[b]), e - 1, n)] if e > 0 else [Fraction(0)] * n
            assert gx[b].tolist() == [float(v) for v in fr_vjp(fr(ga[b]), kern, nx)], (e, b)
    # compose: dh / df_i = g^i, dh_k / dg_j = f'(g)_{k-j}
    gf, gg = grads(lambda f, g: series.compose(f, g, n), xa, ya)
    for b in range(B):
        f, g = fr(xa[b]), fr(ya[b])
        assert gf[b].tolist() == [float(sum(u * v for u, v in zip(fr(ga[b]), fr_pow(g, i, n)))) for i in range(nx)], b
        fp = [Fraction(0)] * n
        for j in range(1, nx):
            fp = [u + j * f[j] * v for u, v in zip(fp, fr_pow(g, j - 1, n))]
        assert gg[b].tolist() == [float(v) for v in fr_vjp(fr(ga[b]), fp, n)], b


# ---- finite differences ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("form", ["A", "B"])
@pytest.mark.parametrize("op", ["mul", "div", "exp", "log", "exp_device_seed", "log_device_seed", "compose", "pow"])
def test_gradcheck(op, form):
    from genfer_amd import series

    B, n, nx = 2, 5, 3
    xa, ya = operands(B, n, nx, second_shape=(n,))  # the second operand broadcast from shape [n]
    xa[:, 0] += 1.0
    x, y = dev(xa, True), dev(ya, True)
    series.set_form(form)
    base = op.split("_")[0]
    if base in BINARY:
        assert torch.autograd.gradcheck(lambda a, b: call(base, a, b, n), (x, y))
    else:
        assert torch.autograd.gradcheck(lambda a: call(base, a, None, n, seeded=not op.endswith("device_seed")), (x,))
    series.set_form(None)


# ---- the documented sequences, bit for bit -----------------------------------------------------------------------------------------


def sequence(op, x, y, gz, n, result):
    """section 4 of the design with explicit public calls on detached tensors: (gx, gy)"""
    from genfer_amd import series

    one = torch.ones(1, dtype=torch.float64, device=DEV)
    nx = x.shape[-1]
    if op == "mul":
        return series.corr(gz, y, nx), series.corr(gz, x, y.shape[-1])
    if op == "div":
        u = series.corr(gz, series.div(one, y, n), n)
        return u[..., :nx], -series.corr(u, result, y.shape[-1])
    if op == "exp":
        return series.corr(gz, result, nx), None
    if op == "log":
        return series.corr(gz, series.div(one, x, n), nx), None
    if op == "pow":
        return 5 * series.corr(gz, series.pow(x, 4, n), nx), None
    fp = x[..., 1:] * torch.arange(1, nx, dtype=torch.float64, device=DEV)
    return series._compose_adj(gz, y, nx), series.corr(gz, series.compose(fp, y, n), y.shape[-1])


@pytest.mark.parametrize("B,n", [(300, 16), (3, 100)])
@pytest.mark.parametrize("op", OPS)
def test_backward_is_the_documented_sequence(op, B, n):
    nx = n - 3
    xa, ya = operands(B, n, nx)
    xa[:, 0] += 1.0
    ga = dense((B, n), 7 * n + B) - 1.0
    x, y, gz = dev(xa, True), dev(ya, op in BINARY), dev(ga)
    z = call(op, x, y, n)
    z.backward(gz)
    with torch.no_grad():
        gx, gy = sequence(op, x.detach(), y.detach(), gz, n, z.detach())
    assert torch.equal(bits(x.grad), bits(gx)), op
    if op in BINARY:
        assert torch.equal(bits(y.grad), bits(gy)), op
    else:
        assert y.grad is None


# ---- against an independent model --------------------------------------------------------------------------------------------------
# the six operations as plain loops over torch CPU float64 tensors (a batch a column), differentiated by torch itself


def m_mul(x, y, n):
    nx, ny = x.shape[-1], y.shape[-1]
    cols = []
    for k in range(n):
        lo, hi = max(0, k + 1 - ny), min(k + 1, nx)
        if hi <= lo:
            cols.append(torch.zeros(x.shape[:-1], dtype=torch.float64))
        else:
            cols.append((x[..., lo:hi] * y[..., k - hi + 1:k - lo + 1].flip(-1)).sum(-1))
    return torch.stack(cols, -1)


def m_div(x, y, n):
    nx, ny = x.shape[-1], y.shape[-1]
    r = []
    for k in range(n):
        lo = max(0, k + 1 - ny)
        c = x[..., k] if k < nx else torch.zeros(x.shape[:-1], dtype=torch.float64)
        if k > lo:
            c = c - (torch.stack(r[lo:k], -1) * y[..., 1:k - lo + 1].flip(-1)).sum(-1)
        r.append(c / y[..., 0])
    return torch.stack(r, -1)


def m_exp(x, n):
    nx = x.shape[-1]
    e = [torch.exp(x[..., 0])]
    for k in range(1, n):
        hi = min(k, nx - 1)
        s = torch.zeros(x.shape[:-1], dtype=torch.float64)
        if hi >= 1:
            j = torch.arange(1, hi + 1, dtype=torch.float64)
            s = (x[..., 1:hi + 1] * j * torch.stack(e[k - hi:k], -1).flip(-1)).sum(-1)
        e.append(s / k)
    return torch.stack(e, -1)


def m_log(x, n):
    nx = x.shape[-1]
    r = [torch.log(x[..., 0])]
    for k in range(1, n):
        lo = max(1, k + 1 - nx)
        c = x[..., k] if k < nx else torch.zeros(x.shape[:-1], dtype=torch.float64)
        if k > lo:
            j = torch.arange(lo, k, dtype=torch.float64)
            c = c - (torch.stack(r[lo:k], -1) * j * x[..., 1:k - lo + 1].flip(-1)).sum(-1) / k
        r.append(c / x[..., 0])
    return torch.stack(r, -1)


def m_compose(f, g, n):
    nf = f.shape[-1]
    res = f[..., nf - 1:nf]
    for i in range(nf - 2, -1, -1):
        res = m_mul(res, g, min(res.shape[-1] + g.shape[-1] - 1, n))
        res = torch.cat([(res[..., 0] + f[..., i]).unsqueeze(-1), res[..., 1:]], -1)
    return torch.cat([res, torch.zeros(res.shape[:-1] + (n - res.shape[-1],), dtype=torch.float64)], -1)


def m_pow(x, e, n):
    r = x
    for _ in range(e - 1):
        r = m_mul(r, x, min(r.shape[-1] + x.shape[-1] - 1, n))
    return torch.cat([r, torch.zeros(r.shape[:-1] + (n - r.shape[-1],), dtype=torch.float64)], -1)


def model(op, x, y, n):
    return {"mul": lambda: m_mul(x, y, n), "div": lambda: m_div(x, y, n), "exp": lambda: m_exp(x, n), "log": lambda: m_log(x, n),
            "compose": lambda: m_compose(x, y, n), "pow": lambda: m_pow(x, 5, n)}[op]()


_model_inputs = {}


def model_inputs(B, n):
    """0.5 + uniform rows, made once per shape and left unchanged"""
    if (B, n) not in _model_inputs:
        _model_inputs[B, n] = (dense((B, n), 11 * n + B), dense((B, n), 13 * n + B), dense((B, n), 17 * n + B))
    return _model_inputs[B, n]


@pytest.mark.parametrize("B,n", [(3, 16), (300, 16), (3, 80), (2, 300)])
@pytest.mark.parametrize("op", OPS)
def test_gradients_against_the_model(op, B, n):
    xa, ya, ga = model_inputs(B, n)
    if op == "compose":
        xa = xa[:, :8]  # nf = 8
    # the model, on the CPU
    xc, yc = torch.from_numpy(xa.copy()).requires_grad_(), torch.from_numpy(ya.copy()).requires_grad_(op in BINARY)
    model(op, xc, yc, n).backward(torch.from_numpy(ga))
    # the library (device seeds: the model's exp / log of coefficient 0 are torch's)
    x, y = dev(xa, True), dev(ya, op in BINARY)
    call(op, x, y, n, seeded=False).backward(dev(ga))
    pairs = [("first", x.grad.cpu(), xc.grad)] + ([("second", y.grad.cpu(), yc.grad)] if op in BINARY else [])
    for which, got, want in pairs:
        assert got.shape == want.shape
        scale = want.abs().amax(dim=-1, keepdim=True)  # every row, against its own largest gradient
        err = (got - want).abs()
        worst = float((err / scale).max())
        print(f"{op} ({B}, {n}) {which}: worst row error {worst:.3e} of the row's largest gradient")
        assert bool((err <= REL_TOL * scale).all()), (op, B, n, which, worst)


# ---- other cases -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("op", OPS)
def test_expanded_grad_output_and_broadcast_operand(op):
    """z.sum().backward() hands over an expanded scalar; the gradient of a stride-0 operand is the batch sum of the per-item ones"""
    B, n, nx = 70, 12, 9
    xa, ya = operands(B, n, nx, second_shape=(n,))
    xa[:, 0] += 1.0
    x, y = dev(xa, True), dev(ya, op in BINARY)
    call(op, x, y, n).sum().backward()
    ones = torch.ones((B, n), dtype=torch.float64, device=DEV)
    x2, y2 = dev(xa, True), dev(np.repeat(ya[None], B, axis=0), op in BINARY)  # the same items, nothing broadcast
    call(op, x2, y2, n).backward(ones)
    assert torch.equal(bits(x.grad), bits(x2.grad))
    if op in BINARY:
        assert y.grad.shape == (n,)
        want = y2.grad.sum(0)
        assert bool(((y.grad - want).abs() <= REL_TOL * want.abs().max()).all())
    # one series of x against a batch of second operands
    if op in BINARY:
        x1, yb = dev(xa[0], True), dev(np.repeat(ya[None], B, axis=0) + dense((B, n), 3) / n)
        call(op, x1, yb, n).backward(ones)
        xr = dev(np.repeat(xa[:1], B, axis=0), True)
        call(op, xr, yb, n).backward(ones)
        assert x1.grad.shape == (nx,)
        want = xr.grad.sum(0)
        assert bool(((x1.grad - want).abs() <= REL_TOL * want.abs().max()).all())


def test_only_the_needed_gradient_is_computed(monkeypatch):
    from genfer_amd import series

    B, n, nf = 300, 16, 8  # 300 items of 16 coefficients: corr takes form A here, the transposed Horner loop has form B only
    fa, ga = operands(B, n, nf)
    gz = torch.ones((B, n), dtype=torch.float64, device=DEV)
    f, g = dev(fa, True), dev(ga)
    h = series.compose(f, g, n)
    series.corr(gz, g)
    assert series.last_form() == "A"
    h.backward(gz)
    assert series.last_form() == "B" and g.grad is None  # the last call was _compose_adj: no corr for g's gradient behind it
    f2, g2 = dev(fa), dev(ga, True)
    h = series.compose(f2, g2, n)
    monkeypatch.setattr(series, "_compose_adj", lambda *a, **k: pytest.fail("the gradient of f was not asked for"))
    h.backward(gz)
    assert series.last_form() == "A" and f2.grad is None and g2.grad is not None
    # mul: one corr call a needed gradient
    calls = []
    real = series.corr
    monkeypatch.setattr(series, "corr", lambda *a, **k: (calls.append(a[1].data_ptr()), real(*a, **k))[1])
    x, y = dev(fa, True), dev(ga)
    series.mul(x, y, n).backward(gz)
    assert calls == [y.data_ptr()] and y.grad is None
    calls.clear()
    x, y = dev(fa, True), dev(ga, True)
    series.mul(x, y, n).backward(gz)
    assert len(calls) == 2
