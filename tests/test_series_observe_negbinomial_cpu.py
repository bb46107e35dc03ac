"""The fused negative-binomial observation and the Lah row (observe_negbinomial of genfer_amd.series, series2, interval_series,
interval_series2; lah_row of series and interval_series) without a GPU: the numpy model of
tests/_series_observe_negbinomial_model.py against the reference's own sequence on the oracle's handle API bit for bit, stored shape
included, the row's recurrence against plain Python floats, the exported surface, the ctypes argument lists, every refusal made
before a device is touched, the host argument layer as a stand-alone program, and the gfx950 code of the kernels."""
import ctypes as C
import glob
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _series_observe_model as M
import _series_observe_negbinomial_model as NM
from _series2_oracle import bits_equal
from conftest import ROOT, splitmix64_uniform

SYMBOLS = tuple(f"{pre}{rank}_observe_negbinomial" for pre in ("gft_", "gfti_") for rank in ("series", "series2")) + ("gft_series_lah_row", "gfti_series_lah_row")
ITEMS = ((5,), (9,), (17,), (33,), (5, 7), (7, 5), (1, 9), (9, 1), (12, 12))
XS = (0.3, -1.7, 1.0, 0.0, -0.0)
PS = (0.25, 0.5, 0.9, 1.0)
PAIRS = tuple(itertools.product(XS, PS))  # one item each
B = len(PAIRS)


def operands(item, K, seed, interval, positive):
    """data without exact zeros, mixed-sign in [-0.5, 0.5) or positive in [0.25, 1.25); x and p: the pairs of XS and PS; a dense row in
    [0.25, 1.25) with a 1.0 at entry 0 of every other item"""
    u = splitmix64_uniform(seed, B * int(np.prod(item))).reshape((B,) + item) + (0.25 if positive else -0.5)
    assert (u != 0.0).all()
    x, p = np.array([q[0] for q in PAIRS]), np.array([q[1] for q in PAIRS])
    ls = 0.25 + splitmix64_uniform(seed + 5, B * (K + 1)).reshape(B, K + 1)
    ls[1::2, 0] = 1.0
    if not interval:
        return u, x, p, ls
    wide = lambda v: np.where((v == 0.0) | (v == 1.0), v, v + 1e-3 * np.abs(v))  # noqa: E731  (points at 0, -0 and 1)
    li = np.stack([ls, ls * (1.0 + 1e-6)])
    li[:, 1::2, 0] = 1.0
    return np.stack([u, u + 1e-3 * np.abs(u)]), np.stack([x, wide(x)]), np.stack([p, wide(p)]), li


def grid(length):
    """(K, degree_p1): K in {0, 1, 2, 5, L - 3}, degree_p1 in {3, 4, L - K}; K >= degree_p1 occurs from L = 9 on (P_i is truncated)"""
    return [(k, d) for k in sorted({0, 1, 2, 5, length - 3}) for d in sorted({3, 4, length - k}) if k >= 0 and d >= 3 and d + k <= length]


def check(got, want, what, items=None):
    assert got.shape == want.shape, f"{what}: shape {got.shape}, the oracle stores {want.shape}"
    ok = bits_equal(got, want)
    assert ok.all(), f"{what}: {(~ok).sum()} coefficients differ, first at {tuple(np.argwhere(~ok)[0])}"


# ---- the model against the oracle ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("item", ITEMS, ids=lambda s: "x".join(map(str, s)))
def test_model_is_the_oracle(OTP, OTPI, item, interval):
    """on data without exact zeros the stated loops are the reference's sequence (zero_with, from * var, from * var_at_zero,
    subst_var, *, add_scaled, derivative, truncate_to_degree_p1), stored shape included, for x in {0.3, -1.7, 1, 0, -0} times p in
    {0.25, 0.5, 0.9, 1}, a dense row and the Lah row.  The f64 Lah row at p == 1 and K >= 1 is all zeros, where the oracle's sum stays
    the one-coefficient zero: there the model must give +0.0 everywhere"""
    T, A = (OTPI, M.IV) if interval else (OTP, M.F64)
    lead = 1 if interval else 0
    rank, cases, truncated = len(item), 0, False
    p_one = np.array([q[1] == 1.0 for q in PAIRS])
    for var in ((0,) if rank == 1 else (0, 1)):
        axis = -1 if rank == 1 else var - 2
        for K, d in grid(item[var]):
            truncated = truncated or K >= d
            for positive in (False, True):
                a, x, p, ls = operands(item, K, 11 + 7 * item[var] + K + d, interval, positive)
                what = f"{item} var={var} K={K} degree_p1={d} {'positive' if positive else 'mixed'}"
                check(NM.observe_negbinomial(A, a, axis, x, p, ls, d, rank), NM.oracle_negbinomial(T, a, item, var, x, p, ls, d, interval), what)
                cases += 1
                if positive:
                    continue
                lah = NM.lah_row(A, p, K)
                got = NM.observe_negbinomial(A, a, axis, x, p, lah, d, rank)
                keep = np.ones(B, dtype=bool) if K == 0 or interval else ~p_one  # ([1, 1] - [1, 1] is widened: no exact zero)
                sel = (slice(None),) * lead + (keep,)
                check(got[sel], NM.oracle_negbinomial(T, a[sel], item, var, x[sel], p[sel], lah[sel], d, interval), what + " lah_row")
                if K >= 1 and not interval:
                    z = got[(slice(None),) * lead + (p_one,)]
                    assert (z == 0.0).all() and not np.signbit(z).any(), what
    assert cases >= 2 and (truncated or max(item) < 9)


def test_grid_truncates_the_power():
    """K >= degree_p1 occurs, so that P_i is cut at degree_p1 coefficients"""
    for L in (9, 17, 33, 12):
        assert any(k >= d for k, d in grid(L)), L
    assert all(d >= 3 and k + d <= 5 for k, d in grid(5)) and len(grid(5)) >= 4


def test_model_on_what_the_oracle_is_no_yardstick_for():
    """the definition where the reference's Mul looks at the data: a zero entry of the row touches the first element only, -0.0
    counts as zero, p == 0 leaves the constant coefficient of every pass, and planted zeros, inf and NaN run the same sequence"""
    a = np.array([[1.0, -2.0, 3.0, -4.0, 5.0, 6.0], [0.0, -0.0, np.inf, 1.0, np.nan, 2.0], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    x, p = np.array([0.5, -0.0, 2.0]), np.array([0.5, 0.25, 0.0])
    ls = np.array([[0.0, -0.0, 0.0], [1.0, -3.0, 1.0], [1.0, 1.0, 1.0]])
    got = NM.observe_negbinomial(M.F64, a, -1, x, p, ls, 4, 1)
    assert got.shape == (3, 4) and (got[0] == 0.0).all() and not np.signbit(got[0]).any()
    assert np.isnan(got[1]).any()
    # p == 0: c = m = 0, pf = [1, 0, 0, 0], P_1 = [0, 0], P_2 = [0, 0, 0]: pass i leaves D_i[0] * 1 in coefficient 0 of pass 0 alone
    assert got[2].tolist() == [1.0, 0.0, 0.0, 0.0]
    # by hand, K = 1, x = 0.5, p = 0.5, ls = [2, 3]: c = 0.25, m = 0.5; S = D * [1, .5, .25]; pass 1: U[j] = S[j-1] * m + c * S[j];
    # sum[j] = (0 + 2 * S_0[j]) + 3 * U_1[j]
    one = NM.observe_negbinomial(M.F64, a[:1, :4], -1, x[:1], p[:1], np.array([[2.0, 3.0]]), 3, 1)
    S0 = [1.0, -2.0 * 0.5, 3.0 * 0.25]
    D1 = [-2.0, 6.0, -12.0]
    S1 = [D1[0], D1[1] * 0.5, D1[2] * 0.25]
    U1 = [0.0 + 0.25 * S1[0], S1[0] * 0.5 + 0.25 * S1[1], S1[1] * 0.5 + 0.25 * S1[2]]
    assert one.tolist() == [[(0.0 + 2.0 * S0[j]) + 3.0 * U1[j] for j in range(3)]]
    ai = np.stack([a, a])
    goti = NM.observe_negbinomial(M.IV, ai, -1, np.stack([x, x]), np.stack([p, p]), np.stack([ls, ls]), 4, 1)
    assert (goti[:, 0] == 0.0).all() and not np.signbit(goti[:, 0]).any()


@pytest.mark.parametrize("order", [0, 1, 2, 7, 20])
def test_lah_row_model(OTP, OTPI, order):
    """the row's model is the recurrence in plain Python floats; the interval model on point intervals encloses it, on [1, 1] and
    [0, 0] keeps its exact entries, and both models are the oracle's scalars"""
    ps = [0.25, 0.5, 0.9, 1.0, 0.0, 1e-3, -0.5]
    got = NM.lah_row(M.F64, np.array(ps), order)
    assert got.shape == (len(ps), order + 1)
    for b, p in enumerate(ps):
        assert got[b].tolist() == NM.lah_row_floats(p, order), p
    check(got, NM.oracle_lah_row(OTP, np.array(ps), order, False), f"order {order}")
    pi = np.stack([np.array(ps), np.array(ps)])
    goti = NM.lah_row(M.IV, pi, order)
    assert goti.shape == (2, len(ps), order + 1)
    assert (goti[0] <= got).all() and (got <= goti[1]).all()
    check(goti, NM.oracle_lah_row(OTPI, pi, order, True), f"order {order} interval")
    wide = np.stack([np.array(ps[:3]), np.array(ps[:3]) * (1.0 + 1e-9)])
    check(NM.lah_row(M.IV, wide, order), NM.oracle_lah_row(OTPI, wide, order, True), f"order {order} wide intervals")
    if order >= 1:  # p == 1: every entry is (1 - 1) / d times something finite (the interval [1, 1] - [1, 1] is widened, not zero)
        assert (got[3] == 0.0).all() and (goti[0, 3] <= 0.0).all() and (goti[1, 3] >= 0.0).all()


# ---- the surface ------------------------------------------------------------------------------------------------------------------


def built_lib():
    import genfer_amd

    if not os.path.exists(genfer_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return genfer_amd.lib()


def test_symbols_are_declared_and_exported():
    """the six entry points: declared in the header, exported; no gftb_, series3_ or series2_lah_row spelling"""
    L = built_lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len(set(SYMBOLS)) == 6
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert hasattr(L, s), s
        assert f"pub fn {s}(" in doc, s
    for s in ("gftb_series_observe_negbinomial", "gftb_series_lah_row", "gft_series3_observe_negbinomial", "gft_series2_lah_row", "gfti_series2_lah_row"):
        assert not hasattr(L, s) and s not in header, s
    from genfer_amd import interval_series, interval_series2, series, series2, series2_grad

    for mod in (series, series2, interval_series, interval_series2):
        assert callable(mod.observe_negbinomial), mod.__name__
    assert callable(series.lah_row) and callable(interval_series.lah_row)
    assert not hasattr(series2, "lah_row") and not hasattr(interval_series2, "lah_row")
    assert not hasattr(series2_grad, "observe_negbinomial") and not hasattr(series2_grad, "lah_row")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_extern.py"), "--check"])


def test_argument_lists_come_from_the_one_table():
    """the ctypes declarations of the six entry points are built from the OPS rows and match the header's parameter lists; the rows
    are MORE_OPS, behind the table OPS (which ends with the affine substitutions and mirrors gft::SERIES_OPS), and leave RANK3 and
    BIGFLOAT_OPS alone"""
    from genfer_amd import _series_call as S

    built_lib()
    L = S._lib()
    assert list(S.OPS)[-2:] == ["mul_linear", "compose_linear"] and list(S.MORE_OPS) == ["observe_negbinomial", "lah_row"]
    op = S.MORE_OPS["observe_negbinomial"]
    assert op.kind == "negbin" and op.long == "x" and op.var and op.names == ("a", "x", "ls")
    assert S.MORE_OPS["lah_row"].kind == "lah" and S.MORE_OPS["lah_row"].long == "result" and S.MORE_OPS["lah_row"].names[0] == "p"
    assert S.RANK3 == ("mul", "div", "exp", "log", "compose", "pow") and S.BIGFLOAT_OPS == ("mul", "div", "exp", "log", "compose", "pow")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    ctype = {"const double*": C.c_void_p, "double*": C.c_void_p, "void*": C.c_void_p, "const int64_t*": S._I64P, "const size_t*": S._SZP,
             "int64_t": C.c_int64, "size_t": C.c_size_t, "int": C.c_int}
    for s in SYMBOLS:
        params = re.search(r"\bint\s+" + s + r"\s*\(([^)]*)\)", header).group(1).split(",")
        want = [ctype[re.sub(r"\s+", " ", p.strip()).rsplit(" ", 1)[0]] for p in params]
        f = getattr(L, s)
        assert f.restype is C.c_int and list(f.argtypes) == want, s
    assert len(L.gft_series_observe_negbinomial.argtypes) == 17 and len(L.gft_series2_observe_negbinomial.argtypes) == 22
    assert len(L.gfti_series_lah_row.argtypes) == 8


def test_modules_import_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "from genfer_amd import series, series2, interval_series, interval_series2\n"
            "assert callable(series.observe_negbinomial) and callable(interval_series2.observe_negbinomial) and callable(interval_series.lah_row)\n"
            "print('ok')")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_bench_series_observe_negbinomial_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_series_observe_negbinomial.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "--shapes" in out.stdout and "--rounds" in out.stdout and "--interval" in out.stdout


# ---- refusals that need no device -------------------------------------------------------------------------------------------------


def modules():
    from genfer_amd import interval_series, interval_series2, series, series2

    return {"series": (series, 1, 0), "series2": (series2, 2, 0), "interval_series": (interval_series, 1, 1),
            "interval_series2": (interval_series2, 2, 1)}


@pytest.mark.parametrize("name", ["series", "series2", "interval_series", "interval_series2"])
def test_refusals_need_no_device(name):
    torch = pytest.importorskip("torch")
    from genfer_amd.taylor import TaylorError

    mod, rank, planes = modules()[name]
    lead = (2,) * planes
    item = (9,) if rank == 1 else (4, 9)
    ones = lambda *s: torch.ones(lead + s, dtype=torch.float64)  # noqa: E731
    a, x, p, ls = ones(3, *item), ones(3), ones(3), ones(3, 3)
    va = (1,) if rank == 2 else ()
    f = lambda a=a, x=x, p=p, ls=ls, va=va, **kw: mod.observe_negbinomial(a, *va, x, p, ls, **kw)  # noqa: E731
    what = rf"{name}\.observe_negbinomial: "
    for d in (2, 1, 0, -3):
        with pytest.raises(TaylorError, match=what + rf"degree_p1 = {d} \(the result needs at least three"):
            f(degree_p1=d)
    with pytest.raises(TaylorError, match=what + r"degree_p1 = 2 .*the default is 9 - order"):
        f(ls=ones(3, 8))
    with pytest.raises(TaylorError, match=what + r"ls holds no entry"):
        f(ls=ones(3, 0))
    with pytest.raises(TaylorError, match=what + r"degree_p1 \+ order = 8 \+ 2, but a has 9 stored coefficients"):
        f(degree_p1=8)
    with pytest.raises(TaylorError, match=what + r"degree_p1 \+ order = 3 \+ 7, but a has 9"):
        f(ls=ones(3, 8), degree_p1=3)
    for bad in (1.5, True, "3"):
        with pytest.raises(TypeError, match="degree_p1 must be an integer"):
            f(degree_p1=bad)
    if rank == 2:
        for var in (2, -1, True, None, 0.0):
            with pytest.raises(TaylorError, match="var = .*is 0 .* or 1"):
                f(va=(var,))
        with pytest.raises(TaylorError, match=r"degree_p1 \+ order = 3 \+ 2, but a has 4 stored coefficients on axis -2"):
            f(va=(0,), degree_p1=3)
        with pytest.raises(TaylorError, match="at least"):
            f(a=ones(9))
    with pytest.raises(TaylorError, match="a: .*is empty"):
        f(a=a[..., :0])
    with pytest.raises(TaylorError, match="a: .*unit stride"):
        f(a=ones(3, *item[:-1], 18)[..., ::2])
    with pytest.raises(TaylorError, match="ls: .*unit stride"):
        f(ls=ones(3, 6)[..., ::2])
    with pytest.raises(TaylorError, match="ls has no axis of entries"):
        f(ls=ones())
    # the shapes of x, p, ls and out
    with pytest.raises(TaylorError, match=r"the batch shapes do not broadcast: a has \(3,\), x has \(2,\), p has \(3,\), ls has \(3,\)"):
        f(x=ones(2))
    with pytest.raises(TaylorError, match=r"the batch shapes do not broadcast: .*p has \(4,\)"):
        f(p=ones(4))
    with pytest.raises(TaylorError, match=r"the batch shapes do not broadcast: .*ls has \(4,\)"):
        f(ls=ones(4, 3))
    res = (7,) if rank == 1 else (4, 7)
    with pytest.raises(TaylorError, match="out has shape"):
        f(out=ones(3, *item))
    with pytest.raises(TaylorError, match="out has shape"):
        f(out=ones(3, *res), degree_p1=5)
    with pytest.raises(TaylorError, match=r"out has batch shape \(2,\)"):
        f(out=ones(2, *res))
    if rank == 2:  # the other axis is cut to min(len, degree_p1)
        with pytest.raises(TaylorError, match=r"the result has \(3, 3\) coefficients per item"):
            f(out=ones(3, 4, 3), degree_p1=3)
    # dtype and type
    for k in ("a", "x", "p", "ls"):
        with pytest.raises(TaylorError, match=f"{k}: .*float32"):
            f(**{k: {"a": a, "x": x, "p": p, "ls": ls}[k].float()})
        with pytest.raises(TypeError, match=f"{k}: expected a torch.Tensor"):
            f(**{k: [[1.0]]})
    with pytest.raises(TaylorError, match="out: .*float32"):
        f(out=ones(3, *res).float())
    if planes:
        with pytest.raises(TaylorError, match=r"p: .*stacked \[2, \.\.\.\]"):
            f(p=torch.ones(3, dtype=torch.float64))
    # the limits bound the operand; the operation's own limit bounds 3 * degree_p1 + order
    limit, own = (2048, 4096) if planes else (4096, 8192)
    big = ones(limit + 1) if rank == 1 else ones(limit // 64 + 1, 64)
    with pytest.raises(TaylorError, match=what + f"a has .*exceeds the limit of {limit}"):
        f(a=big, x=ones(), p=ones(), ls=ones(2))
    if rank == 1:
        d = own // 3 + 1
        with pytest.raises(TaylorError, match=what + rf"3 \* degree_p1 \+ order = 3 \* {d} \+ 1 exceeds the limit of {own}"):
            f(a=ones(limit), x=ones(), p=ones(), ls=ones(2), degree_p1=d)
    at = ones(limit) if rank == 1 else ones(limit // 64, 64)
    # everything in order: broadcasts of x, p and ls, out= -- the placement is judged last
    for kw in ({}, {"x": ones(), "p": ones(), "ls": ones(3)}, {"out": ones(3, *res)}, {"a": at, "x": ones(), "ls": ones(9), "degree_p1": 56},
               {"degree_p1": 3}, {"ls": ones(3, 1)}):
        with pytest.raises(TaylorError, match="a: the tensor is on cpu"):
            f(**kw)


@pytest.mark.parametrize("name", ["series", "interval_series"])
def test_lah_row_refusals_need_no_device(name):
    torch = pytest.importorskip("torch")
    from genfer_amd.taylor import TaylorError

    mod, _, planes = modules()[name]
    lead = (2,) * planes
    ones = lambda *s, **k: torch.ones(lead + s, dtype=torch.float64, **k)  # noqa: E731
    what = rf"{name}\.lah_row: "
    limit = 2048 if planes else 4096
    with pytest.raises(TaylorError, match=what + r"order = -1"):
        mod.lah_row(ones(3), -1)
    with pytest.raises(TaylorError, match=what + rf"order \+ 1 = {limit + 1} exceeds the limit of {limit}"):
        mod.lah_row(ones(3), limit)
    for bad in (1.5, True, "3", None):
        with pytest.raises(TypeError, match="order must be an integer"):
            mod.lah_row(ones(3), bad)
    with pytest.raises(TaylorError, match="p: .*float32"):
        mod.lah_row(ones(3).float(), 2)
    with pytest.raises(TypeError, match="p: expected a torch.Tensor"):
        mod.lah_row([0.5], 2)
    with pytest.raises(TaylorError, match=r"out has shape .*the result has 3 entries per item"):
        mod.lah_row(ones(3), 2, out=ones(3, 4))
    with pytest.raises(TaylorError, match=r"out has batch shape \(2,\); p has \(3,\)"):
        mod.lah_row(ones(3), 2, out=ones(2, 3))
    with pytest.raises(TaylorError, match="out: .*unit stride"):
        mod.lah_row(ones(3), 2, out=ones(3, 6)[..., ::2])
    if planes:
        with pytest.raises(TaylorError, match=r"p: .*stacked \[2, \.\.\.\]"):
            mod.lah_row(torch.ones(3, dtype=torch.float64), 2)
    with pytest.raises(TaylorError, match=what + "p requires grad, and lah_row has no autograd"):
        mod.lah_row(ones(3, requires_grad=True), 2)
    for kw in ({}, {"out": ones(3, 3)}):
        with pytest.raises(TaylorError, match="p: the tensor is on cpu"):
            mod.lah_row(ones(3), 2, **kw)
    with pytest.raises(TaylorError, match="p: the tensor is on cpu"):
        mod.lah_row(ones(), limit - 1)


@pytest.mark.parametrize("name", ["series", "series2", "interval_series", "interval_series2"])
def test_tracked_operands_are_refused_by_name(name):
    """no autograd in this version, in all four modules: a tracked a, x, p or ls under grad mode is refused by its name"""
    torch = pytest.importorskip("torch")
    from genfer_amd.taylor import TaylorError

    mod, rank, planes = modules()[name]
    lead = (2,) * planes
    item = (9,) if rank == 1 else (4, 9)
    va = (1,) if rank == 2 else ()
    mk = lambda *s, g=False: torch.ones(lead + s, dtype=torch.float64, requires_grad=g)  # noqa: E731
    for who in ("a", "x", "p", "ls"):
        a, x, p, ls = mk(3, *item, g=who == "a"), mk(3, g=who == "x"), mk(3, g=who == "p"), mk(3, 3, g=who == "ls")
        with pytest.raises(TaylorError, match=rf"{name}\.observe_negbinomial: {who} requires grad, and observe_negbinomial has no autograd"):
            mod.observe_negbinomial(a, *va, x, p, ls)
        with pytest.raises(TaylorError, match="degree_p1 = 2"):  # the shape rules come first
            mod.observe_negbinomial(a, *va, x, p, ls, degree_p1=2)
        with torch.no_grad():
            with pytest.raises(TaylorError, match="on cpu"):
                mod.observe_negbinomial(a, *va, x, p, ls)


# ---- the host argument layer ----------------------------------------------------------------------------------------------------


def test_series_args_on_the_negative_binomial_observation(tmp_path):
    """tests/series_observe_negbinomial_args_main.cpp: a plain host program over gft_series_args.hpp -- every new refusal's whole
    message and their order, the rank-3 and BigFloat texts in front of them, the strides of x, p and ls in the collapsed batch, the
    overlaps, the Lah row's one rule.  Built with the host compiler and run as its own executable, once plain and once under
    AddressSanitizer and UndefinedBehaviorSanitizer where the compiler has them and the program starts with them"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "onb_args")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "genfer_amd", "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "series_observe_negbinomial_args_main.cpp")]
    ran = 0
    for extra in ([], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]):
        if subprocess.run(base + extra, capture_output=True).returncode != 0:
            assert extra, "tests/series_observe_negbinomial_args_main.cpp does not build"
            continue
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        if extra and out.returncode != 0 and "FAILED" not in out.stdout and "ERROR: " not in out.stderr:
            continue  # (the sanitizers' runtime does not start here: the plain build has decided)
        assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
        m = re.search(r"^ok (\d+) checks$", out.stdout.strip().splitlines()[-1])
        assert m and int(m.group(1)) >= 60, out.stdout
        ran += 1
    assert ran >= 1


# ---- the kernels' code ------------------------------------------------------------------------------------------------------------


def test_series_observe_negbinomial_isa(tmp_path):
    """The gfx950 code of the eight kernels (observation: two forms per element type; the Lah row likewise): no scratch, no spills,
    no calls, no static LDS; the observation's kernels have no f64 FMA and no division (the row's kernels divide by from(d), whose
    expansion holds FMAs); form A exchanges values between lanes (ds_bpermute_b32) without LDS or barrier, form B goes through ds
    reads and writes around a barrier"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"),
                           os.path.join(ROOT, "tests", "series_observe_negbinomial_isa_check.hip")], cwd=tmp_path)
    isa = open(glob.glob(str(tmp_path / "*amdgcn-amd-amdhsa*gfx950*.s"))[0]).read()
    assert isa.count(".private_segment_fixed_size: 0") == 8 and isa.count(".private_segment_fixed_size:") == 8
    assert isa.count(".amdhsa_group_segment_fixed_size 0\n") == 8
    assert isa.count(".vgpr_spill_count: 0") == 8  # (scalar registers may move into vector lanes: the by-value batch is large)
    kernels = {}
    for m in re.finditer(r"^(_ZN3gft\w+):[^\n]*\n(.*?)^\.Lfunc_end", isa, flags=re.S | re.M):
        kernels[m.group(1)] = [ln.split()[0] for ln in m.group(2).splitlines() if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((".", ";"))]
    assert len(kernels) == 8
    for name, code in kernels.items():
        assert len(code) > 30, name
        assert not [c for c in code if c.startswith(("scratch_", "buffer_", "flat_"))], name
        assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")], name
        # (the row's workgroup kernel reads its one p at a uniform address: a scalar load)
        assert any(c.startswith("global_load") for c in code) or "k_lah_row_lds" in name, name
        assert any(c.startswith("global_store") for c in code), name
        assert any(c.startswith("v_mul_f64") for c in code) and any(c.startswith("v_add_f64") for c in code), name
        if "k_obs_negbin" in name:
            assert not [c for c in code if ("fma" in c and "f64" in c) or c.startswith("v_div_")], name
        else:
            assert any(c.startswith("v_div_") for c in code), name
        lds = [c for c in code if c.startswith("ds_") and "permute" not in c]
        if name.split("INS_")[0].endswith("_wave"):
            assert not lds and "s_barrier" not in code, name
            assert any(c.startswith("ds_bpermute_b32") for c in code), name
        else:
            assert any(c.startswith("ds_read") for c in lds) and any(c.startswith("ds_write") for c in lds) and "s_barrier" in code, name
