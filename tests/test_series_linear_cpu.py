"""The batched affine substitutions (mul_linear and compose_linear of genfer_amd.series, series2, interval_series, interval_series2;
gft[i]_series[2]_mul_linear / _compose_linear) without a GPU: the numpy model of tests/_series_linear_model.py against the oracle's
handle API bit for bit, stored shape included (mul_linear, and subst_var with the affine series [c, m]), the exported surface, the
ctypes argument lists, every refusal made before a device is touched, the host argument layer as a stand-alone program, and the
gfx950 code of the kernels."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _series_linear_model as LM
import _series_observe_model as M
from _series2_oracle import bits_equal
from conftest import ROOT, splitmix64_uniform

OPS = ("mul_linear", "compose_linear")
SYMBOLS = tuple(f"{pre}{rank}_{op}" for pre in ("gft_", "gfti_") for rank in ("series", "series2") for op in OPS)
CS = (0.0, -0.0, 1.0, 0.3, -1.7)  # one item each
MS = (1.7, 0.5, 1.0, -0.4, 0.9)
B = len(CS)
ITEMS1 = ((1,), (2,), (3,), (4,), (7,), (12,))
ITEMS2 = ((5, 7), (7, 5), (1, 5), (5, 1), (2, 2), (3, 4), (4, 3), (6, 6))


def operands(item, seed, interval):
    """data without exact zeros in [-0.5, 0.5); c and m: the five pairs of CS and MS.  Intervals: [v, v + w] not reaching zero, c a point
    at 0, -0 and 1, m a point at 1"""
    u = splitmix64_uniform(seed, B * int(np.prod(item))).reshape((B,) + item) - 0.5
    assert (u != 0.0).all()
    c, m = np.array(CS), np.array(MS)
    if not interval:
        return u, c, m
    wd = 1e-3 * np.abs(u)
    a = np.stack([u, np.where(u < 0.0, np.minimum(u + wd, -1e-300), u + wd)])
    assert ((a[0] <= a[1]) & ((a[0] > 0.0) | (a[1] < 0.0))).all()
    ci = np.stack([c, c + np.array([0.0, 0.0, 0.0, 1e-3, 1e-3])])
    mi = np.stack([m, m + np.array([1e-3, 1e-4, 0.0, 1e-3, 1e-3])])
    return a, ci, mi


def orders(item, w):
    """four result shapes per item: the least one (two on w), one more, a longer one and (9, 9)"""
    rank = len(item)
    least = tuple(max(k, 2) if i == w else k for i, k in enumerate(item))
    more = tuple(k + 1 for k in least)
    longer = tuple(k + (3, 2)[i % 2] for i, k in enumerate(least))
    return sorted({least, more, longer, (9,) * rank if all(k <= 9 for k in item) else tuple(k + 5 for k in item)})


def check(got, want, what):
    assert got.shape == want.shape, f"{what}: shape {got.shape}, the oracle stores {want.shape}"
    ok = bits_equal(got, want)
    assert ok.all(), f"{what}: {(~ok).sum()} coefficients differ, first at {tuple(np.argwhere(~ok)[0])}"


# ---- the model against the oracle ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("item", ITEMS1 + ITEMS2, ids=lambda s: "x".join(map(str, s)))
def test_model_is_the_oracle(OTP, OTPI, item, interval):
    """on data without exact zeros the stated loops are the oracle's mul_linear and its subst_var with the affine series [c, m] on
    axis w, stored shape included; c holds 0, -0, 1 and ordinary values in one batch, every (v, w) and four orders per item"""
    T, A = (OTPI, M.IV) if interval else (OTP, M.F64)
    rank, cases = len(item), 0
    for v in range(rank):
        for w in range(rank):
            for n in orders(item, w):
                a, c, m = operands(item, 3 + 11 * item[0] + 5 * item[-1] + v + 2 * w, interval)
                what = f"{item} v={v} w={w} n={n}"
                got = LM.compose_linear(A, a, v, c, m, w, n, rank)
                assert got.shape[-rank:] == LM.compact_shape("compose_linear", item, v, w, n)
                check(got, LM.oracle_linear(T, "compose_linear", a, item, v, w, c, m, n, interval), "compose_linear " + what)
                if v == w:
                    got = LM.mul_linear(A, a, w, c, m, n[w], rank)
                    check(got, LM.oracle_linear(T, "mul_linear", a, item, v, w, c, m, n, interval), "mul_linear " + what)
                cases += 1
    assert cases >= 3


def test_model_on_what_the_oracle_is_no_yardstick_for():
    """the definition where the reference's Mul looks at the data: planted zeros, -0.0, inf and NaN run the same sequence, -0.0 counts as
    zero for c, and absent terms are absent"""
    a = np.array([[1.0, -2.0, 3.0], [-0.0, np.inf, -1.0], [0.0, np.nan, 2.0]])
    c, m = np.array([0.5, -0.0, 2.0]), np.array([2.0, -3.0, 0.0])
    got = LM.mul_linear(M.F64, a, 0, c, m, 4, 1)
    assert got.shape == (3, 4)
    assert got[0].tolist() == [0.0 + 0.5 * 1.0, 1.0 * 2.0 + 0.5 * -2.0, -2.0 * 2.0 + 0.5 * 3.0, 3.0 * 2.0]
    # item 1, c == -0.0: t alone -- position 0 is +0.0, no c * a[j] (inf * -0.0 would be NaN)
    assert got[1, 0] == 0.0 and not np.signbit(got[1, 0]) and got[1, 2] == -np.inf and not np.isnan(got[1]).any()
    assert np.isnan(got[2, 1]) and np.isnan(got[2, 2])  # 2 * nan, nan * 0
    # compose_linear by hand: f(0.5 + 2 t) = f0 + f1 (0.5 + 2t) + f2 (0.5 + 2t)^2, Horner with mul_linear
    r = LM.compose_linear(M.F64, a[:1], 0, c[:1], m[:1], 0, (3,), 1)
    s1 = [0.0 + 0.5 * 3.0, 3.0 * 2.0]
    s1[0] = s1[0] + -2.0
    s2 = [0.0 + 0.5 * s1[0], s1[0] * 2.0 + 0.5 * s1[1], s1[1] * 2.0]
    s2[0] = s2[0] + 1.0
    assert r.tolist() == [s2]
    # c == -0.0 on the replaced variable: the power table, slice i times m^i, with slice 0 times 1.0 (so -0.0 stays -0.0)
    p = LM.compose_linear(M.F64, a[1:2], 0, c[1:2], m[1:2], 0, (5,), 1)
    assert p.shape == (1, 3) and np.signbit(p[0, 0]) and p[0, 1] == -np.inf and p[0, 2] == -9.0
    ai = np.stack([a, a])
    pi = LM.compose_linear(M.IV, ai, 0, np.stack([c, c]), np.stack([m, m]), 0, (3,), 1)
    # [-3, -3]^2 is widened by an ulp each way, times the point -1: negated, no second widening
    assert pi.shape == (2, 3, 3) and pi[0, 1, 2] == np.nextafter(-9.0, -np.inf) and pi[1, 1, 2] == np.nextafter(-9.0, 0.0)
    assert LM.padded(M.F64, p, (5,), 1).tolist() == [[-0.0, -np.inf, -9.0, 0.0, 0.0]]


# ---- the surface ------------------------------------------------------------------------------------------------------------------


def built_lib():
    import genfer_amd

    if not os.path.exists(genfer_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return genfer_amd.lib()


def test_symbols_are_declared_and_exported():
    """the eight entry points: declared in the header, exported; the four modules have the functions and the
    differentiable twin does not"""
    L = built_lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len(set(SYMBOLS)) == 8
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert hasattr(L, s), s
        assert f"pub fn {s}(" in doc, s
    from genfer_amd import interval_series, interval_series2, series, series2, series2_grad

    for mod in (series, series2, interval_series, interval_series2):
        assert callable(mod.mul_linear) and callable(mod.compose_linear), mod.__name__
    assert not hasattr(series2_grad, "mul_linear") and not hasattr(series2_grad, "compose_linear")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_extern.py"), "--check"])


def test_argument_lists_come_from_the_one_table():
    """the ctypes declarations of the eight entry points are built from the OPS rows and match the header's parameter lists"""
    from genfer_amd import _series_call as S

    built_lib()
    L = S._lib()
    for name, nvar in (("mul_linear", 1), ("compose_linear", 2)):
        op = S.OPS[name]
        assert op.kind == "linear" and op.long == "result" and op.var == nvar
    assert S.RANK3 == ("mul", "div", "exp", "log", "compose", "pow") and S.F64_ONLY == ("corr", "compose_adj")
    assert list(S.OPS)[-2:] == ["mul_linear", "compose_linear"]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    ctype = {"const double*": C.c_void_p, "double*": C.c_void_p, "void*": C.c_void_p, "const int64_t*": S._I64P, "const size_t*": S._SZP,
             "int64_t": C.c_int64, "size_t": C.c_size_t, "int": C.c_int}
    for s in SYMBOLS:
        params = re.search(r"\bint\s+" + s + r"\s*\(([^)]*)\)", header).group(1).split(",")
        want = [ctype[re.sub(r"\s+", " ", p.strip()).rsplit(" ", 1)[0]] for p in params]
        f = getattr(L, s)
        assert f.restype is C.c_int and list(f.argtypes) == want, s
    assert len(L.gft_series_mul_linear.argtypes) == 13 and len(L.gft_series2_mul_linear.argtypes) == 18
    assert len(L.gfti_series_compose_linear.argtypes) == 13 and len(L.gfti_series2_compose_linear.argtypes) == 19


def test_modules_import_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "from genfer_amd import series, series2, interval_series, interval_series2\n"
            "assert callable(series.compose_linear) and callable(interval_series2.mul_linear)\nprint('ok')")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_bench_series_linear_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_series_linear.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "--rows" in out.stdout and "--rounds" in out.stdout and "--out" in out.stdout


# ---- refusals that need no device -------------------------------------------------------------------------------------------------


def modules():
    from genfer_amd import interval_series, interval_series2, series, series2

    return {"series": (series, 1, 0), "series2": (series2, 2, 0), "interval_series": (interval_series, 1, 1),
            "interval_series2": (interval_series2, 2, 1)}


@pytest.mark.parametrize("opname", OPS)
@pytest.mark.parametrize("name", ["series", "series2", "interval_series", "interval_series2"])
def test_refusals_need_no_device(name, opname):
    torch = pytest.importorskip("torch")
    from genfer_amd.taylor import TaylorError

    mod, rank, planes = modules()[name]
    comp = opname == "compose_linear"
    lead = (2,) * planes
    item = (9,) if rank == 1 else (4, 9)
    ones = lambda *s: torch.ones(lead + s, dtype=torch.float64)  # noqa: E731
    a, c, m = ones(3, *item), ones(3), ones(3)
    va = (1,) if rank == 2 else ()
    fn = getattr(mod, opname)
    f = lambda a=a, c=c, m=m, va=va, **kw: fn(a, *va, c, m, **kw)  # noqa: E731
    what = rf"{name}\.{opname}: "
    an = "f" if comp else "a"
    pair = lambda k: k if rank == 1 else (4, k)  # noqa: E731
    # a result of one coefficient on the axis is no linear substitution
    with pytest.raises(TaylorError, match=what + r"the result has 1 coefficient.*needs two"):
        f(a=ones(3, *item[:-1], 1), n=pair(1))
    if comp:  # the default order is the stored shape: one coefficient on the axis is refused, not widened
        with pytest.raises(TaylorError, match=what + r"the result has 1 coefficient"):
            f(a=ones(3, *item[:-1], 1))
    if rank == 2:
        for var in (2, -1, True, None, 0.0):
            with pytest.raises(TaylorError, match=what + "var = .*is 0 .* or 1"):
                f(va=(var,))
        if comp:
            for wv in (2, -1, True, 0.5):
                with pytest.raises(TaylorError, match=what + "wvar = .*is 0 .* or 1"):
                    f(wvar=wv)
            with pytest.raises(TaylorError, match=what + r"the result has 1 coefficient on axis -2"):
                f(wvar=0, n=(1, 12))
        with pytest.raises(TaylorError, match="at least"):
            f(a=ones(9))
        with pytest.raises(TaylorError, match=what + r"n = \(5,\); the order of a bivariate result is a pair"):
            f(n=(5,))
    with pytest.raises(TaylorError, match=what + an + r" has .* coefficients, the result n = .*longer than the truncation order"):
        f(n=pair(8))
    limit = 2048 if planes else 4096
    with pytest.raises(TaylorError, match=what + rf"n = .* exceeds the limit of {limit} coefficients per"):
        f(n=limit + 1 if rank == 1 else (limit // 64 + 1, 64))
    for bad in (1.5, "3"):
        with pytest.raises(TypeError, match="n must be"):
            f(n=bad)
    with pytest.raises(TaylorError, match=an + ": .*is empty"):
        f(a=a[..., :0])
    with pytest.raises(TaylorError, match=an + ": .*unit stride"):
        f(a=ones(3, *item[:-1], 18)[..., ::2])
    # the scalars have the batch shape
    with pytest.raises(TaylorError, match=rf"the batch shapes do not broadcast: {an} has \(3,\), c has \(2,\), m has \(3,\)"):
        f(c=ones(2))
    with pytest.raises(TaylorError, match=r"the batch shapes do not broadcast: .*m has \(4,\)"):
        f(m=ones(4))
    res = pair(10) if not comp else pair(9)
    res = (res,) if rank == 1 else res
    with pytest.raises(TaylorError, match="out has shape"):
        f(out=ones(3, *res), n=pair(12))
    with pytest.raises(TaylorError, match=r"out has batch shape \(2,\)"):
        f(out=ones(2, *res))
    for k in (an, "c", "m"):
        kw = "a" if k == an else k
        with pytest.raises(TaylorError, match=f"{k}: .*float32"):
            f(**{kw: {"a": a, "c": c, "m": m}[kw].float()})
        with pytest.raises(TypeError, match=f"{k}: expected a torch.Tensor"):
            f(**{kw: [[1.0]]})
    with pytest.raises(TaylorError, match="out: .*float32"):
        f(out=ones(3, *res).float())
    if planes:
        with pytest.raises(TaylorError, match=r"c: .*stacked \[2, \.\.\.\]"):
            f(c=torch.ones(3, dtype=torch.float64))
    at = ones(limit - 1) if rank == 1 else ones(limit // 64, 63)
    # everything in order: broadcasts of c and m (stride 0 included), out=, the limit itself -- the placement is judged last
    # (wvar != var: the default orders hold f's own length on var, so f lies inside them)
    for kw in ({}, {"c": ones(), "m": ones()}, {"c": ones(1).expand(*lead, 3)}, {"out": ones(3, *res)}, {"n": pair(12)},
               {"a": at, "c": ones(), "m": ones(), "n": limit if rank == 1 else (limit // 64, 64)}) + (({"wvar": 0},) if comp and rank == 2 else ()):
        with pytest.raises(TaylorError, match=an + ": the tensor is on cpu"):
            f(**kw)


@pytest.mark.parametrize("opname", OPS)
@pytest.mark.parametrize("name", ["series", "series2", "interval_series", "interval_series2"])
def test_tracked_operands_are_refused_by_name(name, opname):
    """no autograd in this version, in all four modules: a tracked operand, c or m under grad mode is refused by its name"""
    torch = pytest.importorskip("torch")
    from genfer_amd.taylor import TaylorError

    mod, rank, planes = modules()[name]
    lead = (2,) * planes
    item = (9,) if rank == 1 else (4, 9)
    va = (1,) if rank == 2 else ()
    fn = getattr(mod, opname)
    an = "f" if opname == "compose_linear" else "a"
    mk = lambda *s, g=False: torch.ones(lead + s, dtype=torch.float64, requires_grad=g)  # noqa: E731
    for who in (an, "c", "m"):
        a, c, m = mk(3, *item, g=who == an), mk(3, g=who == "c"), mk(3, g=who == "m")
        with pytest.raises(TaylorError, match=rf"{name}\.{opname}: {who} requires grad, and {opname} has no autograd"):
            fn(a, *va, c, m)
        with pytest.raises(TaylorError, match="longer than the truncation order"):  # the shape rules come first
            fn(a, *va, c, m, n=8 if rank == 1 else (4, 8))
        with torch.no_grad():
            with pytest.raises(TaylorError, match="on cpu"):
                fn(a, *va, c, m)


# ---- the host argument layer ----------------------------------------------------------------------------------------------------


def test_series_args_on_affine_substitutions(tmp_path):
    """tests/series_linear_args_main.cpp: a plain host program over gft_series_args.hpp -- the refusals in C with their texts, the
    strides of c and m in the collapsed batch, the overlaps, the unchanged rank-3 refusal, the empty batch; under AddressSanitizer and
    UndefinedBehaviorSanitizer where the compiler has them and the program runs with them"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lin_args")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "genfer_amd", "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "series_linear_args_main.cpp")]
    for extra in (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []):
        if subprocess.run(base + extra, capture_output=True).returncode != 0:
            continue
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        if extra and out.returncode != 0 and "FAILED" not in out.stdout:
            continue  # (the sanitizers' runtime does not start here: the plain build decides)
        assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
        mm = re.search(r"^ok (\d+) checks$", out.stdout.strip().splitlines()[-1])
        assert mm and int(mm.group(1)) >= 40, out.stdout
        return
    pytest.fail("tests/series_linear_args_main.cpp does not build")


# ---- the kernels' code ------------------------------------------------------------------------------------------------------------

VGPRS = {"k_lin_mul": (28, 42), "k_lin_compose_wave": (34, 61), "k_lin_compose_lds": (28, 53)}  # (f64, interval): what DESIGN 3.27 records


def test_series_linear_isa(tmp_path):
    """The gfx950 code of the six kernels (mul_linear and compose's two forms per element type): no scratch, no calls, no f64 FMA, no
    division and no flat access; form A and the streaming kernel allocate no LDS, form A exchanges values between lanes
    (ds_bpermute_b32); form B has no static LDS (its two line buffers are dynamic) and goes through ds reads and writes around a
    barrier.  The VGPR counts stay within what DESIGN 3.27 records."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", "series_linear_isa_check.hip")],
                          cwd=tmp_path)
    isa = open(glob.glob(str(tmp_path / "*amdgcn-amd-amdhsa*gfx950*.s"))[0]).read()
    assert isa.count(".private_segment_fixed_size: 0") == 6 and isa.count(".private_segment_fixed_size:") == 6
    assert isa.count(".amdhsa_group_segment_fixed_size 0\n") == 6
    assert isa.count(".vgpr_spill_count: 0") == 6
    kernels = {}
    for mm in re.finditer(r"^(_ZN3gft\w+):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M):
        kernels[mm.group(1)] = [ln.split()[0] for ln in mm.group(2).splitlines() if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((".", ";"))]
    assert len(kernels) == 6
    vgprs = {mm.group(1): int(mm.group(2)) for mm in re.finditer(r"\.name:\s+(_ZN3gft\w+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", isa)}
    for name, code in kernels.items():
        assert len(code) > 30, name
        assert not [c for c in code if c.startswith(("scratch_", "buffer_", "flat_"))], name
        assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")], name
        assert not [c for c in code if ("fma" in c and "f64" in c) or c.startswith("v_div_")], name
        assert any(c.startswith("global_load") for c in code) and any(c.startswith("global_store") for c in code), name
        assert any(c.startswith("v_mul_f64") for c in code) and any(c.startswith("v_add_f64") for c in code), name
        lds = [c for c in code if c.startswith("ds_") and "permute" not in c]
        kind = next(k for k in VGPRS if k in name)
        if kind == "k_lin_compose_lds":
            assert any(c.startswith("ds_read") for c in lds) and any(c.startswith("ds_write") for c in lds) and "s_barrier" in code, name
        else:
            assert not lds and "s_barrier" not in code, name
            assert (kind == "k_lin_mul") != any(c.startswith("ds_bpermute_b32") for c in code), name
        assert name in vgprs and vgprs[name] <= VGPRS[kind]["EIv" in name], (name, vgprs.get(name))
