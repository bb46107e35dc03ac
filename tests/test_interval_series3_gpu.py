"""Batched trivariate interval series on device tensors (genfer_amd.interval_series3, gfti_series3_*) on the MI355X.

Every bound of every coefficient of every item is compared bit for bit (a NaN for a NaN) with the oracle's Interval<F64>: the raw
product of tests/series3_interval_oracle.cpp for mul, the handle operators for div / exp / log where they are normative and the
model of tests/_series3_interval_model.py elsewhere and on small items, 3.23's chains over that product for compose and pow (all
pinned to each other on the CPU by tests/test_interval_series3_cpu.py).  The stored result shape and its squeezes, views, in-place
results, refusals at both layers, the limit, the stream contract, and point intervals enclosing the f64 family's results."""
import ctypes as C

import numpy as np
import pytest

import _series3_compose_cases as cc
from _series3_model import result_shape
from conftest import REL_TOL
from test_interval_series3_cpu import (assert_bits, data3, host_seeds, is_normative, shim3, want_compose, want_handle, want_model,  # noqa: F401
                                       want_mul, want_pow)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 0x5A5A5A5A5A5A5A5A
OPS = ("mul", "div", "exp", "log")
ALL = OPS + ("compose", "pow")
KINDS = ("dense", "signed", "special")
# minimal; odd N (the unpaired middle output); (8, 8, 8): more coefficients than lanes in rec (the stride loop); (8, 8, 16): N = 1024,
# more output pairs than lanes in mul, pass 1 chunked (7 * 8 terms of 128 elements against the 3072 left of 80 KB); the limit with
# 16 KB of scratch left (eight slabs of 128 elements at (16, 16, 8), the one slab of 1024 at (2, 2, 512): tc = 8 and 1); the limit through the squeezes (rank 2 with s2_div1d's block form, rank 1)
SHAPES = [(2, 2, 2), (3, 4, 5), (5, 3, 2), (8, 8, 8), (8, 8, 16), (16, 16, 8), (2, 2, 512), (1, 1, 2048), (2048, 1, 1), (1, 2048, 1), (2, 1024, 1),
          (2, 1, 1024)]
# stored unit axes under longer result axes, so that S != n; every squeeze of S (3.22's lists, tests/test_series3_gpu.py)
S_CASES = [((4, 2, 1), (5, 3, 2), (5, 3, 2)), ((4, 2, 2), (4, 1, 2), (4, 3, 2)), ((2, 2, 1), (2, 1, 1), (4, 3, 2)), ((1, 3, 2), (2, 1, 2), (3, 3, 3)),
           ((3, 3, 3), (1, 1, 1), (3, 3, 3)), ((2, 3, 1), (1, 1, 1), (3, 3, 2))]
SQUEEZES = [(3, 1, 4), (3, 4, 1), (1, 3, 4), (4, 1, 1), (1, 1, 5), (1, 1, 1)]
MODEL_MAX = 64  # coefficients per item the scalar model is used on (every step is a ctypes call)


@pytest.fixture(scope="module", autouse=True)
def _init():
    import genfer_amd

    genfer_amd.init(0)
    yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64)


def ivs3():
    from genfer_amd import interval_series3

    return interval_series3


LDS_REFUSALS = []


def run(op, X, Y, n, seeds=None, **kw):
    """X: numpy [2, B, nx0, nx1, nx2] or a tensor; Y likewise (mul, div).  Where the runtime grants only 64 KB of LDS an item that
    needs more is refused by name; that refusal is returned as None (and recorded), anything else raises"""
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    tx = X if isinstance(X, torch.Tensor) else dev(X)
    try:
        if op in ("mul", "div"):
            got = getattr(ivs3(), op)(tx, Y if isinstance(Y, torch.Tensor) else dev(Y), n=n, **kw)
        else:
            got = getattr(ivs3(), op)(tx, n=n, seed=None if seeds is None else dev(seeds), **kw)
    except TaylorError as e:
        if "bytes of LDS" in str(e) and "of two bounds" in str(e) and "the runtime grants 65536 bytes" in str(e):
            LDS_REFUSALS.append((op, n))
            return None
        raise
    assert series.last_form() == "B"
    return got


def needs_more_than_64k(op, n, xs, ys):
    """the resident operand, the result (on S, permuted: the unit axes in front) and the smallest scratch, 16 bytes an element"""
    s = result_shape(op, n, xs, ys)
    order = [i for i in range(3) if s[i] == 1] + [i for i in range(3) if s[i] != 1]
    p, a = [s[i] for i in order], [(ys if op == "div" else xs)[i] for i in order]
    need = (p[2] if min(p[1], a[1]) > 1 else 0) if p[0] == 1 else p[1] * p[2]
    return op != "mul" and (int(np.prod(a)) + int(np.prod(s)) + need) * 16 > 65536


def expected(op, X, Y, n, OTPI, oracle_lib, shim):
    """(the expected value, who supplied it, the host seeds)"""
    seeds = host_seeds(oracle_lib, op, X) if op in ("exp", "log") else None
    if op == "mul":
        return want_mul(shim, X, Y, n), "oracle", None
    if is_normative(op, X, Y):
        return want_handle(OTPI, op, X, Y, n), "oracle", seeds
    assert int(np.prod(n)) <= MODEL_MAX, (op, n)
    return want_model(oracle_lib, op, X, Y, n, seeds), "model", seeds


# ---- bit-exact against the oracle ------------------------------------------------------------------------------------------------


def operand_shapes(op, n, kind):
    """dense, and the compact operands of tests/_series3_compose_cases.compact_shapes.  Where the oracle is not normative (a divisor of
    one stored coefficient; exp of a single row or column with special values) items of at most MODEL_MAX coefficients go to the
    model and larger ones keep that operand dense and finite"""
    out = [(n, n)]
    xs, ys = cc.compact_shapes(n)
    if op == "div" and int(np.prod(ys)) == 1 and int(np.prod(n)) > MODEL_MAX:
        ys = n
    if (xs, ys) != (n, n):
        out.append((xs, ys))
    return out


def kind_for(op, n, kind, xs):
    if op == "exp" and kind == "special" and sum(v > 1 for v in xs) <= 1 and int(np.prod(n)) > MODEL_MAX:
        return "signed"
    return kind


@pytest.mark.parametrize("op", OPS)
def test_bit_exact_against_the_oracle(op, OTPI, oracle_lib, shim3):
    checked = {"oracle": 0, "model": 0}
    big_ran, big_refused = [], []  # the cases whose arrays and smallest scratch exceed 64 KB
    for i, n in enumerate(SHAPES):
        N = int(np.prod(n))
        for k0 in (KINDS if N <= 64 else (KINDS[i % 3],)):
            for xs, ys in operand_shapes(op, n, k0):
                kind = kind_for(op, n, k0, xs)
                B = 5 if N <= 64 else (3 if N <= 1024 else 2)  # (the CPU oracle's side of exp / log at the limit is the cost)
                X, Y = data3(kind, B, xs, 1000 * n[0] + 10 * n[1] + n[2] + B), data3(kind, B, ys, 2000 * n[0] + 10 * n[1] + n[2] + B + 7)
                expect, by, seeds = expected(op, X, Y, n, OTPI, oracle_lib, shim3)
                got = run(op, X, Y, n, seeds)
                if got is None:  # refused by name under a 64 KB grant: only an item whose arrays and smallest scratch exceed it
                    assert needs_more_than_64k(op, n, xs, ys), (op, n, xs, ys)
                    big_refused.append((n, xs, ys))
                    continue
                assert_bits(got, expect, f"{op} n={n} B={B} x{xs} y{ys} {kind} against the {by}")
                checked[by] += B
                if needs_more_than_64k(op, n, xs, ys):
                    big_ran.append((n, xs, ys))
    print(f"{op}: items checked {checked}; cases above 64 KB of LDS: {len(big_ran)} ran, {len(big_refused)} refused under a 64 KB grant")
    assert checked["oracle"] >= 90, checked
    # the grant is one value per process and element type: either every case above 64 KB ran (an 80 KB grant: nothing may be refused,
    # and the limit shapes are among those that ran) or every one was refused by name -- a planner that refuses wrongly is not hidden
    assert not (big_ran and big_refused), (big_ran, big_refused)
    # (the four: full operands at the limit with a second slab or row -- (16, 16, 8), (2, 2, 512), (2, 1024, 1), (2, 1, 1024))
    assert len(big_ran) + len(big_refused) == (0 if op == "mul" else 4), (big_ran, big_refused)


@pytest.mark.parametrize("op", OPS)
def test_stored_result_shape_and_squeezes(op, OTPI, oracle_lib, shim3):
    by = {"oracle": 0, "model": 0}
    differs = 0
    for j, (xs, ys, n) in enumerate(S_CASES + [(n, n, n) for n in SQUEEZES]):
        kind = KINDS[(j + 2) % 3]  # (special values on the single row (1, 1, 5): exp's class for the model)
        X, Y = data3(kind, 3, xs, 100 * n[0] + sum(xs)), data3(kind, 3, ys, 200 * n[1] + sum(ys))
        expect, who, seeds = expected(op, X, Y, n, OTPI, oracle_lib, shim3)
        got = run(op, X, Y, n, seeds)
        assert_bits(got, expect, f"{op} x{xs} y{ys} n={n} {kind} against the {who}")
        by[who] += 3
        s = result_shape(op, n, xs, ys)
        differs += s != n
        outside = got.cpu().numpy().copy()
        outside[:, :, :s[0], :s[1], :s[2]] = 0.0
        assert not outside.any() and not np.signbit(outside).any(), (op, n, "outside S is [+0.0, +0.0]")
    assert differs >= 1 and by["oracle"] >= 24 and (by["model"] > 0) == (op in ("div", "exp")), by


@pytest.mark.parametrize("op", ["div", "exp", "log"])
def test_small_items_against_the_model(op, oracle_lib):
    """the loops of include/gftaylor.h over the oracle's scalar interval operations, special values included: the definition itself"""
    for n, xs, ys in [((2, 2, 2),) * 3, ((3, 3, 4), (3, 2, 4), (2, 3, 3)), ((3, 4, 5), (3, 4, 5), (1, 1, 1)), ((1, 3, 4), (1, 3, 4), (1, 1, 4)), ((1, 1, 5), (1, 1, 5), (1, 1, 1))]:
        for kind in KINDS:
            X, Y = data3(kind, 5, xs, 31 * n[0] + n[2]), data3(kind, 5, ys, 37 * n[0] + n[2])
            seeds = host_seeds(oracle_lib, op, X) if op != "div" else None
            assert_bits(run(op, X, Y, n, seeds), want_model(oracle_lib, op, X, Y, n, seeds), f"{op} n={n} x{xs} y{ys} {kind}")


def test_batch_of_65_and_empty_batch(OTPI, oracle_lib, shim3):
    n, B = (3, 4, 5), 65
    X, Y = data3("special", B, n, 31), data3("signed", B, n, 37)
    for op in OPS:
        expect, _, seeds = expected(op, X, Y, n, OTPI, oracle_lib, shim3)
        assert_bits(run(op, X, Y, n, seeds), expect, f"{op} n={n} B={B}")
    assert_bits(ivs3().compose(dev(X), dev(Y), 1), want_compose(shim3, oracle_lib, X, Y, 1, n), "compose B=65")
    assert_bits(ivs3().pow(dev(X), 3), want_pow(shim3, X, 3, n), "pow B=65")
    e = torch.zeros((2, 0, 3, 2, 8), dtype=torch.float64, device=DEV)
    m = ivs3()
    for got in (m.mul(e, e), m.div(e, e), m.exp(e), m.log(e), m.compose(e, e, 2), m.pow(e, 3), m.pow(e, 0)):
        assert got.shape == (2, 0, 3, 2, 8)


def test_default_and_explicit_orders(OTPI, oracle_lib, shim3):
    X, Y = data3("signed", 5, (3, 2, 6), 61), data3("signed", 5, (2, 4, 2), 62)
    assert_bits(ivs3().mul(dev(X), dev(Y)), want_mul(shim3, X, Y, (3, 4, 6)), "mul default n")
    assert_bits(ivs3().mul(dev(X), dev(Y), n=(5, 6, 9)), want_mul(shim3, X, Y, (5, 6, 9)), "mul n beyond both")
    assert_bits(ivs3().div(dev(X), dev(Y), n=(4, 5, 7)), want_handle(OTPI, "div", X, Y, (4, 5, 7)), "div n beyond both")
    for op in ("exp", "log"):
        assert_bits(run(op, X, None, (4, 3, 7), host_seeds(oracle_lib, op, X)), want_handle(OTPI, op, X, None, (4, 3, 7)), f"{op} n beyond x")


# ---- device seeds ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,B", [((3, 4, 5), 65), ((1, 3, 4), 3), ((8, 8, 8), 3)])
def test_device_seeds(n, B, OTPI, oracle_lib):
    """only what depends on coefficient [0, 0, 0] may differ: exp within a few ulps everywhere, log at [0, 0, 0] alone"""
    X = data3("dense", B, n, 31 * n[0] + B)
    for op in ("exp", "log"):
        expect = want_handle(OTPI, op, X, None, n)
        assert_bits(run(op, X, None, n, host_seeds(oracle_lib, op, X)), expect, f"{op} n={n} B={B} host seeds")
        got = run(op, X, None, n, None).cpu().numpy()
        if op == "log":
            g, w = got.copy(), expect.copy()
            g[:, :, 0, 0, 0] = w[:, :, 0, 0, 0] = 0.0
            assert_bits(g, w, f"log n={n} B={B} device seed, all but [0, 0, 0]")
            got, expect = got[:, :, :1, :1, :1], expect[:, :, :1, :1, :1]
        assert np.all(np.abs(got - expect) <= REL_TOL * np.abs(expect)), (op, n, B, np.max(np.abs(got - expect) / np.abs(expect)))


# ---- compose and pow ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("var", [0, 1, 2])
def test_compose_bit_exact(var, oracle_lib, shim3):
    """both instantiations -- g resident in LDS at (4, 4, 4), g in global memory at n = (8, 16, 16) with a full g (2 * 2048 + 2048 elements
    of 16 bytes exceed the 80 KB request whatever was granted) -- a compact g, a two-slice and a one-slice f, the squeezes"""
    checked = 0
    for j, n in enumerate([(2, 2, 2), (4, 4, 4), (3, 4, 5), (1, 3, 4), (3, 1, 4), (4, 1, 1)]):
        fc, gc = cc.compact_shapes(n)
        one = tuple(1 if a == var else n[a] for a in range(3))
        for i, (fs, gs) in enumerate([(n, n), (fc, n), (n, gc), (cc.two_slices(n, var), n), (one, n), (n, tuple(min(2, v) for v in n)), (n, (1, 1, 1))]):
            kind = KINDS[(i + j) % 3]
            F, G = data3(kind, 3, fs, 1000 * n[0] + n[2] + var + i), data3(kind, 3, gs, 2000 * n[0] + n[2] + 7 + i)
            assert_bits(ivs3().compose(dev(F), dev(G), var, n=n), want_compose(shim3, oracle_lib, F, G, var, n), f"compose var={var} n={n} f{fs} g{gs} {kind}")
            checked += 3
    n = (8, 16, 16)
    assert (2 * 2048 + 2048) * 16 > 80 * 1024
    B = 2
    fs = cc.two_slices(n, var)
    F, G = data3("signed", B, fs, 83 + var), data3("signed", B, n, 84)
    want = want_compose(shim3, oracle_lib, F, G, var, n)
    assert_bits(ivs3().compose(dev(F), dev(G), var, n=n), want, f"compose var={var} n={n} f{fs}, g in global memory")
    # g in global memory through slab, row and plane strides of its own
    wide = torch.zeros((B, 2, n[0], n[1] + 1, n[2] + 16), dtype=torch.float64, device=DEV)
    gv = wide[..., :n[1], 3:3 + n[2]].movedim(1, 0)
    gv.copy_(dev(G))
    assert gv.stride(0) == n[0] * (n[1] + 1) * (n[2] + 16) and gv.stride(-2) == n[2] + 16
    assert_bits(ivs3().compose(dev(F), gv, var, n=n), want, f"compose var={var} n={n}, strided g in global memory")
    assert checked + 2 * B >= 100


@pytest.mark.parametrize("n,B,kind", [((1, 1, 1), 5, "signed"), ((2, 2, 2), 5, "special"), ((3, 4, 5), 5, "special"), ((1, 3, 4), 3, "dense"),
                                      ((8, 8, 8), 65, "special"), ((8, 8, 16), 3, "signed"), ((2, 1024, 1), 2, "dense")])
def test_pow_bit_exact(n, B, kind, shim3):
    X = data3(kind, B, n, 900 * n[0] + n[2])
    xc = cc.compact_shapes(n)[0]
    Xc = data3(kind, B, xc, 901 * n[0] + n[2])
    for e in (0, 1, 2, 3, 5):
        assert_bits(ivs3().pow(dev(X), e), want_pow(shim3, X, e, n), f"pow n={n} B={B} e={e} {kind}")
        if e in (2, 5) and B <= 5:
            assert_bits(ivs3().pow(dev(Xc), e, n=n), want_pow(shim3, Xc, e, n), f"pow n={n} compact x{xc} e={e}")


# ---- views -----------------------------------------------------------------------------------------------------------------------


def call(op, a, b, seeds, **kw):
    m = ivs3()
    if op in ("mul", "div"):
        return getattr(m, op)(a, b, **kw)
    if op == "compose":
        return m.compose(a, b, 1, **kw)
    if op == "pow":
        return m.pow(a, 3, **kw)
    return getattr(m, op)(a, seed=seeds[op], **kw)


@pytest.mark.parametrize("n,batch", [((3, 4, 5), (4, 5)), ((4, 4, 9), (2, 3))])
def test_views(n, batch, OTPI, oracle_lib, shim3):
    B, nb = int(np.prod(batch)), len(batch)
    X, Y = data3("signed", B, n, 11), data3("signed", B, n, 12)
    full = (2,) + batch + n

    def expect_all(X, Y):
        e = {op: expected(op, X, Y, n, OTPI, oracle_lib, shim3)[0] for op in OPS}
        e["compose"] = want_compose(shim3, oracle_lib, X, Y, 1, n)
        e["pow"] = want_pow(shim3, X, 3, n)
        return {k: v.reshape(full) for k, v in e.items()}

    expect = expect_all(X, Y)
    tX, tY = dev(X).reshape(full), dev(Y).reshape(full)
    seeds = {op: dev(host_seeds(oracle_lib, op, X)).reshape((2,) + batch) for op in ("exp", "log")}
    box = (slice(1, 1 + n[0]), slice(2, 2 + n[1]), slice(4, 4 + n[2]))
    # slab and row strides: a slice of a wider tensor on all three series axes
    wide = torch.zeros((2,) + batch + (n[0] + 2, n[1] + 3, n[2] + 9), dtype=torch.float64, device=DEV)
    wide[(Ellipsis,) + box] = tX
    xs = wide[(Ellipsis,) + box]
    assert xs.stride(-2) == n[2] + 9 and xs.stride(-3) == (n[1] + 3) * (n[2] + 9)
    for op in ALL:
        assert_bits(call(op, xs, tY, seeds), expect[op], f"{op} sliced x")
    # the planes interleaved per item: [B..., 2, n0, n1, n2] in memory
    inter = tX.movedim(0, nb).contiguous().movedim(nb, 0)
    N = int(np.prod(n))
    assert inter.stride(0) == N and inter.stride(nb) == 2 * N
    for op in ALL:
        assert_bits(call(op, inter, tY, seeds), expect[op], f"{op} interleaved planes")
    oi = torch.empty(batch + (2,) + n, dtype=torch.float64, device=DEV).movedim(nb, 0)
    for op in ALL:
        assert call(op, tX, tY, seeds, out=oi) is oi
        assert_bits(oi, expect[op], f"{op} out with interleaved planes")
    # a transposed batch
    perm = (0,) + tuple(reversed(range(1, nb + 1))) + (nb + 1, nb + 2, nb + 3)
    xp = tX.permute(*perm).contiguous().permute(*perm)
    assert not xp.is_contiguous() and xp.stride(-1) == 1
    for op in ALL:
        assert_bits(call(op, xp, tY, seeds), expect[op], f"{op} permuted x")
    # plane stride 0: point intervals, no copy (seeds too)
    P = np.stack([X[0], X[0]])
    pe = dev(X[0]).reshape(batch + n).expand(full)
    assert pe.stride(0) == 0
    ep = expect_all(P, Y)
    ps = {op: dev(host_seeds(oracle_lib, op, P)).reshape((2,) + batch) for op in ("exp", "log")}
    for op in ALL:
        assert_bits(call(op, pe, tY, ps), ep[op], f"{op} x with plane stride 0")
    assert_bits(ivs3().mul(tY, pe), want_mul(shim3, Y, P, n).reshape(full), "mul y with plane stride 0")
    # a stride-0 batch axis: one item against the batch, on either side
    Y0 = np.repeat(Y[:, :1], B, axis=1)
    ye = dev(Y[:, :1]).reshape((2,) + (1,) * nb + n).expand(full)
    assert ye.stride(1) == 0
    assert_bits(ivs3().mul(tX, ye), want_mul(shim3, X, Y0, n).reshape(full), "mul expanded y")
    assert_bits(ivs3().div(tX, dev(Y[:, 0])), want_handle(OTPI, "div", X, Y0, n).reshape(full), "div broadcast y")
    assert_bits(ivs3().div(ye, tX), want_handle(OTPI, "div", Y0, X, n).reshape(full), "div expanded x")
    # an out= view with guard words around it, intact afterwards
    obox = (slice(1, 1 + n[0]), slice(1, 1 + n[1]), slice(2, 2 + n[2]))
    for op in ALL:
        big = torch.full((2,) + batch + (n[0] + 2, n[1] + 2, n[2] + 5), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
        out = big[(Ellipsis,) + obox]
        assert call(op, xs, tY, seeds, out=out) is out
        assert_bits(out, expect[op], f"{op} sliced out")
        g = big.view(torch.int64).clone()
        g[(Ellipsis,) + obox] = GUARD
        assert bool((g == GUARD).all()), op
    # a result whose S is smaller than n through a strided out: the zero fill goes through the strides and both planes
    Xc = data3("dense", B, (2, 2, 1), 13)
    big = torch.full((2,) + batch + (n[0] + 2, n[1] + 2, n[2] + 5), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
    out = big[(Ellipsis,) + obox]
    tc = dev(Xc).reshape((2,) + batch + (2, 2, 1))
    ivs3().mul(tc, tc, n=n, out=out)
    assert_bits(out, want_mul(shim3, Xc, Xc, n).reshape(full), "mul S < n into a sliced out")
    g = big.view(torch.int64).clone()
    g[(Ellipsis,) + obox] = GUARD
    assert bool((g == GUARD).all())
    # in place: the result as the same view of an operand, planes included
    for op in ALL:
        xi = tX.clone()
        assert call(op, xi, tY, seeds, out=xi) is xi
        assert_bits(xi, expect[op], f"{op} in place on x")
        ii = torch.empty_strided(inter.shape, inter.stride(), dtype=torch.float64, device=DEV)
        ii.copy_(inter)
        call(op, ii, tY, seeds, out=ii)
        assert_bits(ii, expect[op], f"{op} in place on interleaved x")
    for op in ("mul", "div", "compose"):
        yi = tY.clone()
        call(op, tX, yi, seeds, out=yi)
        assert_bits(yi, expect[op], f"{op} in place on y")
        wi = wide.clone()
        v = wi[(Ellipsis,) + box]
        call(op, v, tY, seeds, out=v)
        assert_bits(v, expect[op], f"{op} in place on a sliced x")


# ---- refusals and limits -----------------------------------------------------------------------------------------------------------


def test_refusals_and_limits():
    from genfer_amd.taylor import TaylorError

    import genfer_amd

    m = ivs3()
    shape = (2, 6, 2, 4, 16)
    x = torch.rand(shape, dtype=torch.float64, device=DEV) + 0.5
    y = torch.rand(shape, dtype=torch.float64, device=DEV) + 0.5

    def after():  # no stale HIP error: torch's next call succeeds
        assert float((x + 1.0).sum().item()) > 0

    # the Python layer
    with pytest.raises(TaylorError, match=r"n0 \* n1 \* n2 = 3 \* 683 \* 1 = 2049 exceeds the limit of 2048"):
        m.mul(x[..., :1, :1, :1], y[..., :1, :1, :1], n=(3, 683, 1))
    with pytest.raises(TaylorError, match="needs at least 4"):
        m.mul(x[0, 0], y)
    with pytest.raises(TaylorError, match="var = 3"):
        m.compose(x, y, 3)
    with pytest.raises(TaylorError, match="nx > n"):
        m.exp(x, n=(2, 4, 15))
    with pytest.raises(TaylorError, match="no autograd"):
        m.mul(x.clone().requires_grad_(True), y)
    # the library, through the Python layer: the result's planes, slabs, rows and items are distinct addresses
    with pytest.raises(TaylorError, match="zero plane stride"):
        m.mul(x, y, out=torch.empty((1,) + shape[1:], dtype=torch.float64, device=DEV).expand(shape))
    after()
    with pytest.raises(TaylorError, match="zero stride"):
        m.mul(x, y, out=torch.empty((2, 1, 2, 4, 16), dtype=torch.float64, device=DEV).expand(shape))
    with pytest.raises(TaylorError, match="zero slab stride"):
        m.mul(x, y, out=torch.empty((2, 6, 1, 4, 16), dtype=torch.float64, device=DEV).expand(shape))
    with pytest.raises(TaylorError, match="zero row stride"):
        m.mul(x, y, out=torch.empty((2, 6, 2, 1, 16), dtype=torch.float64, device=DEV).expand(shape))
    with pytest.raises(TaylorError, match="overlap"):  # the planes 64 apart, an item 128 long: the planes overlap each other
        m.mul(x, y, out=torch.empty(4096, dtype=torch.float64, device=DEV).as_strided(shape, (64, 128, 64, 16, 1)))
    after()
    buf = torch.rand((2, 6, 2, 4, 40), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps x"):
        m.mul(buf[..., 0:16], y, out=buf[..., 8:24])
    with pytest.raises(TaylorError, match="partially overlaps y"):
        m.div(x, buf[..., 0:16], out=buf[..., 16:32])
    with pytest.raises(TaylorError, match="partially overlaps f"):
        m.compose(buf[..., 0:16], y, 0, out=buf[..., 8:24])
    with pytest.raises(TaylorError, match="partially overlaps x"):  # the same memory with another plane stride is not the same view
        m.exp(buf[:1].expand(2, 6, 2, 4, 40)[..., :16], out=buf[..., :16])
    sd = torch.rand(shape, dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps the seeds"):
        m.exp(x, seed=sd[:, :, 0, 0, 0], out=sd)
    after()
    # the C entry points
    m.mul(x, y)  # declares the entry points
    L = genfer_amd.lib()
    one = (C.c_size_t * 1)(6)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    big = torch.zeros(2 * 6 * 2049, dtype=torch.float64, device=DEV)

    def c_mul(nr, rbs=None):
        return L.gfti_series3_mul(vp(x), None, 64, 16, 2, 4, 16, vp(y), None, 64, 16, 2, 4, 16, vp(big), rbs, nr[1] * nr[2], nr[2], *nr, one, 1, None)

    for nr, rbs, text in [((3, 683, 1), None, "interval series3_mul: n0 * n1 * n2 = 3 * 683 * 1 exceeds the limit of 2048 coefficients per item"),
                          ((2, 0, 16), None, "n0 * n1 * n2 == 0"),
                          ((2, 3, 16), None, "x has 2 x 4 x 16 coefficients, the result 2 x 3 x 16"),
                          ((2, 4, 16), (C.c_int64 * 2)(0, 128), "zero plane stride"),
                          ((2, 4, 16), (C.c_int64 * 2)(-768, 128), "negative strides are not supported (the result, the plane axis)"),
                          ((2, 4, 16), (C.c_int64 * 2)(64, 128), "overlap each other")]:
        assert c_mul(nr, rbs) == -1 and text in L.gft_last_error().decode(), (text, L.gft_last_error())
        after()
    assert L.gfti_series3_exp(vp(x), None, 64, 16, 2, 4, 16, None, None, None, None, 64, 16, 2, 4, 16, one, 1, None) == -1
    assert "interval series3_exp: the result is a null pointer" in L.gft_last_error().decode()
    assert L.gfti_series3_compose(vp(x), None, 64, 16, 2, 4, 16, vp(y), None, 64, 16, 2, 4, 16, 5, vp(big), None, 64, 16, 2, 4, 16, one, 1, None) == -1
    assert "interval series3_compose: var = 5" in L.gft_last_error().decode()
    after()
    assert c_mul((2, 4, 16)) == 0 and c_mul((2, 4, 16), (C.c_int64 * 2)(768, 128)) == 0
    after()
    assert torch.equal(bits(big[:1536].view(2, 6, 2, 4, 16)), bits(m.mul(x, y)))
    # pow's cap on non-contiguous batch axes, by name: ten axes of 2 that alternate between a stride and 0 on x
    xb = torch.rand((2,) + (2, 1) * 5 + (1, 1, 2), dtype=torch.float64, device=DEV).expand((2,) + (2,) * 10 + (1, 1, 2))
    with pytest.raises(TaylorError, match="interval series3_pow: the batch has more than 9 non-contiguous axes"):
        m.pow(xb, 3)
    assert m.mul(xb, xb).shape == xb.shape
    after()
    # the limit itself runs in every orientation, and the calls after the refusals are unharmed
    for n in [(16, 16, 8), (1, 1, 2048), (2048, 1, 1), (1, 2048, 1), (2, 1, 1024), (2, 1024, 1)]:
        a = torch.rand((2, 2) + n, dtype=torch.float64, device=DEV) + 0.5
        assert m.mul(a, a).shape == (2, 2) + n and m.pow(a, 2).shape == (2, 2) + n
    assert torch.equal(bits(m.mul(x, y)), bits(m.mul(x.clone(), y.clone())))


# ---- streams ---------------------------------------------------------------------------------------------------------------------


def test_side_stream_is_ordered_with_torchs_work(shim3):
    B, n = 512, (2, 3, 4)
    X, Y = data3("signed", B, n, 41), data3("signed", B, n, 42)
    expect = want_mul(shim3, X, Y, n)
    tX, tY = dev(X), dev(Y)
    src = torch.zeros((2, B) + n, dtype=torch.float64, device=DEV)
    ivs3().mul(src, tY)  # warm the kernel
    ivs3().pow(src, 3)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(20_000_000)  # the operand is produced behind a long kernel on this stream
        src.copy_(tX)
        z = ivs3().mul(src, tY)
        p = ivs3().pow(src, 3)  # a sequence of launches on pool workspace inside one call
        twice = z * 2.0  # consumed right after, no host synchronisation in between
        src.zero_()  # the operand is reused right after
    s.synchronize()
    assert_bits(z, expect, "mul on a side stream")
    assert_bits(twice, expect * 2.0, "consumer on the side stream")
    assert_bits(p, want_pow(shim3, X, 3, n), "pow on a side stream")


# ---- point intervals enclose f64 ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [(3, 4, 5), (8, 8, 8), (1, 3, 4)])
def test_point_intervals_enclose_the_f64_family(n):
    """x.expand(2, ...) operands: lo <= series3.<op>(x) <= hi elementwise for all six ops, on finite results"""
    from _series3_oracle import dense, signed
    from genfer_amd import series3

    B = 3
    x, y = dev(dense((B,) + n, 51)), dev(signed((B,) + n, 52))
    px, py = x.expand((2, B) + n), y.expand((2, B) + n)
    assert px.stride(0) == 0
    m = ivs3()
    pairs = [("mul", m.mul(px, py), series3.mul(x, y)), ("div", m.div(px, py), series3.div(x, y)), ("exp", m.exp(py * 0.25), series3.exp(y * 0.25)),
             ("log", m.log(px), series3.log(x)), ("pow", m.pow(py, 5), series3.pow(y, 5))]
    pairs += [(f"compose var={v}", m.compose(px, py * 0.25, v), series3.compose(x, y * 0.25, v)) for v in (0, 1, 2)]
    checked = 0
    for name, iv, f in pairs:
        iv, f = iv.cpu().numpy(), f.cpu().numpy()
        fin = np.isfinite(f) & np.isfinite(iv).all(axis=0)
        assert fin.any(), name
        assert np.all(iv[0][fin] <= f[fin]) and np.all(f[fin] <= iv[1][fin]), name
        assert np.all(iv[0][fin] <= iv[1][fin]), name
        checked += int(fin.sum())
    assert checked >= 6 * B * int(np.prod(n))
