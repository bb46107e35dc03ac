"""The fused observation chain (observe_chain of genfer_amd.series, series2, interval_series, interval_series2;
gft[i]_series_observe_chain / gft[i]_series2_observe_chain) without a GPU: the numpy model of tests/_series_observe_chain_model.py
against the oracle's handle API bit for bit (observe_chain for the discrete form, derive_scale step by step for the continuous one),
the exported surface, the ctypes argument lists, every refusal made before a device is touched, the host argument layer as a
stand-alone program, and the gfx950 code of the kernels."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _series_observe_chain_model as CM
import _series_observe_model as M
from _series2_oracle import bits_equal
from conftest import ROOT, splitmix64_uniform

SYMBOLS = tuple(f"{pre}{rank}_observe_chain" for pre in ("gft_", "gfti_") for rank in ("series", "series2"))
ITEMS = ((9,), (33,), (5, 7), (7, 5), (12, 12), (1, 9), (9, 1), (3, 20))
XS = (0.0, -0.0, 1.0, 0.3, -1.7)  # one item each
B = len(XS)


def operands(item, nsteps, seed, interval, with_one):
    """data without exact zeros in [-0.5, 0.5); x: the five scalars of XS; cs in [0.25, 1.25), with 1.0 at step 0 of every other item"""
    u = splitmix64_uniform(seed, B * int(np.prod(item))).reshape((B,) + item) - 0.5
    assert (u != 0.0).all()
    x = np.array(XS)
    cs = 0.25 + splitmix64_uniform(seed + 5, B * nsteps).reshape(B, nsteps)
    if with_one:
        cs[1::2, 0] = 1.0
    if not interval:
        return u, x, cs
    a = np.stack([u, u + 1e-3 * np.abs(u)])
    xi = np.stack([x, x + np.array([0.0, 0.0, 0.0, 1e-3, 1e-3])])
    ci = np.stack([cs, cs * (1.0 + 1e-6)])
    if with_one:
        ci[:, 1::2, 0] = 1.0
    return a, xi, ci


def chains(length):
    """(nsteps, degree_p1) of the grid: 1, 2 and 5 steps, degree_p1 in {2, 3, L - nsteps}"""
    return [(n, d) for n in (1, 2, 5) for d in sorted({2, 3, length - n}) if d >= 2 and d + n <= length]


def check(got, want, what):
    assert got.shape == want.shape, f"{what}: shape {got.shape}, the oracle stores {want.shape}"
    ok = bits_equal(got, want)
    assert ok.all(), f"{what}: {(~ok).sum()} coefficients differ, first at {tuple(np.argwhere(~ok)[0])}"


# ---- the model against the oracle ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("item", ITEMS, ids=lambda s: "x".join(map(str, s)))
def test_model_is_the_oracle(OTP, OTPI, item, interval):
    """on data without exact zeros the stated loops are the oracle's observe_chain (discrete) and its derive_scale applied step by
    step (continuous), stored shape included; x holds 0, -0, 1 and ordinary values, the constants with and without a 1.0"""
    T, A = (OTPI, M.IV) if interval else (OTP, M.F64)
    rank, cases = len(item), 0
    for var in ((0,) if rank == 1 else (0, 1)):
        axis = -1 if rank == 1 else var - 2
        for n, d in chains(item[var]):
            for with_one in (False, True):
                a, x, cs = operands(item, n, 11 + 7 * item[var] + n + d, interval, with_one)
                for xx in (x, None):
                    got = CM.observe_chain(A, a, axis, xx, cs, d, rank)
                    check(got, CM.oracle_chain(T, a, item, var, xx, cs, d, interval), f"{item} var={var} nsteps={n} degree_p1={d} x={'given' if xx is not None else None}")
                    cases += 1
    assert cases >= 4


def test_model_on_what_the_oracle_is_no_yardstick_for():
    """the definition where the reference's Mul looks at the data: a zero constant leaves the item at +0.0 whatever follows, -0.0
    counts as zero for x and c, and planted zeros, inf and NaN run the same sequence"""
    a = np.array([[1.0, -2.0, 3.0, -4.0, 5.0, 6.0], [0.0, -0.0, np.inf, 1.0, np.nan, 2.0]])
    x = np.array([0.5, -0.0])
    cs = np.array([[2.0, -0.0, np.inf], [1.0, -3.0, 1.0]])
    got = CM.observe_chain(M.F64, a, -1, x, cs, 3, 1)
    assert got.shape == (2, 3) and (got[0] == 0.0).all() and not np.signbit(got[0]).any()
    # item 1, x == -0.0: mul_var alone -- position 0 is +0.0 in every step, the others are D[kv - 1] times c
    assert got[1, 0] == 0.0 and not np.signbit(got[1, 0])
    cont = CM.observe_chain(M.F64, a, -1, None, cs, 3, 1)
    assert (cont[0] == 0.0).all() and np.isnan(cont[1]).any()
    # by hand, one step, x = 0.5, c = 2: res[kv] = 2 * ((0 + D[kv-1] * 1) + 0.5 * D[kv]), D[j] = src[j+1] * (j + 1)
    one = CM.observe_chain(M.F64, a[:1, :4], -1, np.array([0.5]), np.array([[2.0]]), 3, 1)
    D = [-2.0, 6.0, -12.0]
    assert one.tolist() == [[2.0 * (0.0 + 0.5 * D[0]), 2.0 * (D[0] + 0.5 * D[1]), 2.0 * (D[1] + 0.5 * D[2])]]
    ai = np.stack([a, a])
    goti = CM.observe_chain(M.IV, ai, -1, np.stack([x, x]), np.stack([cs, cs]), 3, 1)
    assert (goti[:, 0] == 0.0).all() and not np.signbit(goti[:, 0]).any()


# ---- the surface ------------------------------------------------------------------------------------------------------------------


def built_lib():
    import genfer_amd

    if not os.path.exists(genfer_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return genfer_amd.lib()


def test_symbols_are_declared_and_exported():
    """the 16 observation entry points and the four chains: declared in the header, exported, in INTEGRATION.md"""
    plain = ("derivative", "taylor_expansion_of_coeff", "shift_down", "evaluate_all_one")
    PLAIN = tuple(f"{pre}{rank}_{op}" for pre in ("gft_", "gfti_") for rank in ("series", "series2") for op in plain)
    L = built_lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    every = PLAIN + SYMBOLS
    assert len(SYMBOLS) == 4 and len(set(every)) == 20
    for s in every:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert hasattr(L, s), s
        assert f"pub fn {s}(" in doc, s
    from genfer_amd import interval_series, interval_series2, series, series2, series2_grad

    for mod in (series, series2, interval_series, interval_series2):
        assert callable(mod.observe_chain), mod.__name__
    assert not hasattr(series2_grad, "observe_chain")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_extern.py"), "--check"])


def test_argument_lists_come_from_the_one_table():
    """the ctypes declarations of the four entry points are built from the OPS row and match the header's parameter lists"""
    from genfer_amd import _series_call as S

    built_lib()
    L = S._lib()
    op = S.OPS["observe_chain"]
    assert op.kind == "chain" and op.long == "x" and op.var
    assert S.RANK3 == ("mul", "div", "exp", "log", "compose", "pow") and "observe_chain" not in S.F64_ONLY
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    ctype = {"const double*": C.c_void_p, "double*": C.c_void_p, "void*": C.c_void_p, "const int64_t*": S._I64P, "const size_t*": S._SZP,
             "int64_t": C.c_int64, "size_t": C.c_size_t, "int": C.c_int}
    for s in SYMBOLS:
        params = re.search(r"\bint\s+" + s + r"\s*\(([^)]*)\)", header).group(1).split(",")
        want = [ctype[re.sub(r"\s+", " ", p.strip()).rsplit(" ", 1)[0]] for p in params]
        f = getattr(L, s)
        assert f.restype is C.c_int and list(f.argtypes) == want, s
    assert len(L.gft_series_observe_chain.argtypes) == 15 and len(L.gft_series2_observe_chain.argtypes) == 20


def test_modules_import_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "from genfer_amd import series, series2, interval_series, interval_series2\n"
            "assert callable(series.observe_chain) and callable(interval_series2.observe_chain)\nprint('ok')")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_bench_series_observe_chain_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_series_observe_chain.py"), "--help"], capture_output=True, text=True)
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
    a, x, cs = ones(3, *item), ones(3), ones(3, 2)
    va = (1,) if rank == 2 else ()
    f = lambda a=a, x=x, cs=cs, va=va, **kw: mod.observe_chain(a, *va, x, cs, **kw)  # noqa: E731
    what = rf"{name}\.observe_chain: "
    for d in (1, 0, -3):
        with pytest.raises(TaylorError, match=what + rf"degree_p1 = {d} \(the result needs at least two"):
            f(degree_p1=d)
    with pytest.raises(TaylorError, match=what + r"degree_p1 = 1 .*the default is 9 - nsteps"):
        f(cs=ones(3, 8))
    with pytest.raises(TaylorError, match=what + r"nsteps = 0"):
        f(cs=ones(3, 0))
    with pytest.raises(TaylorError, match=what + r"degree_p1 \+ nsteps = 8 \+ 2, but a has 9 stored coefficients"):
        f(degree_p1=8)
    with pytest.raises(TaylorError, match=what + r"degree_p1 \+ nsteps = 2 \+ 8, but a has 9"):
        f(cs=ones(3, 8), degree_p1=2)
    for bad in (1.5, True, "3"):
        with pytest.raises(TypeError, match="degree_p1 must be an integer"):
            f(degree_p1=bad)
    if rank == 2:
        for var in (2, -1, True, None, 0.0):
            with pytest.raises(TaylorError, match="var = .*is 0 .* or 1"):
                f(va=(var,))
        with pytest.raises(TaylorError, match=r"degree_p1 \+ nsteps = 3 \+ 2, but a has 4 stored coefficients on axis -2"):
            f(va=(0,), degree_p1=3)
        with pytest.raises(TaylorError, match="at least"):
            f(a=ones(9))
    with pytest.raises(TaylorError, match="a: .*is empty"):
        f(a=a[..., :0])
    with pytest.raises(TaylorError, match="a: .*unit stride"):
        f(a=ones(3, *item[:-1], 18)[..., ::2])
    with pytest.raises(TaylorError, match="cs: .*unit stride"):
        f(cs=ones(3, 4)[..., ::2])
    with pytest.raises(TaylorError, match="cs has no axis of constants"):
        f(cs=ones())
    # the shapes of x, cs and out
    with pytest.raises(TaylorError, match=r"the batch shapes do not broadcast: a has \(3,\), x has \(2,\), cs has \(3,\)"):
        f(x=ones(2))
    with pytest.raises(TaylorError, match=r"the batch shapes do not broadcast: .*cs has \(4,\)"):
        f(cs=ones(4, 2))
    with pytest.raises(TaylorError, match=r"the batch shapes do not broadcast"):
        f(x=ones(3, 2))  # x has no axis of steps: (3, 2) is a batch shape
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
    for k in ("a", "x", "cs"):
        with pytest.raises(TaylorError, match=f"{k}: .*float32"):
            f(**{k: {"a": a, "x": x, "cs": cs}[k].float()})
        with pytest.raises(TypeError, match=f"{k}: expected a torch.Tensor"):
            f(**{k: [[1.0]]})
    with pytest.raises(TaylorError, match="out: .*float32"):
        f(out=ones(3, *res).float())
    if planes:
        with pytest.raises(TaylorError, match=r"x: .*stacked \[2, \.\.\.\]"):
            f(x=torch.ones(3, dtype=torch.float64))
    # the limits bound the operand
    limit = 2048 if planes else 4096
    big = ones(limit + 1) if rank == 1 else ones(limit // 64 + 1, 64)
    with pytest.raises(TaylorError, match=what + f"a has .*exceeds the limit of {limit}"):
        f(a=big, x=ones(), cs=ones(2))
    at = ones(limit) if rank == 1 else ones(limit // 64, 64)
    # everything in order: broadcasts of x and cs, the continuous form, out= -- the placement is judged last
    for kw in ({}, {"x": None}, {"x": ones(), "cs": ones(2)}, {"out": ones(3, *res)}, {"a": at, "x": ones(), "cs": ones(16)}, {"degree_p1": 2}):
        with pytest.raises(TaylorError, match="a: the tensor is on cpu"):
            f(**kw)


@pytest.mark.parametrize("name", ["series", "series2", "interval_series", "interval_series2"])
def test_tracked_operands_are_refused_by_name(name):
    """no autograd in this version, in all four modules: a tracked a, x or cs under grad mode is refused by its name"""
    torch = pytest.importorskip("torch")
    from genfer_amd.taylor import TaylorError

    mod, rank, planes = modules()[name]
    lead = (2,) * planes
    item = (9,) if rank == 1 else (4, 9)
    va = (1,) if rank == 2 else ()
    mk = lambda *s, g=False: torch.ones(lead + s, dtype=torch.float64, requires_grad=g)  # noqa: E731
    for who in ("a", "x", "cs"):
        a, x, cs = mk(3, *item, g=who == "a"), mk(3, g=who == "x"), mk(3, 2, g=who == "cs")
        with pytest.raises(TaylorError, match=rf"{name}\.observe_chain: {who} requires grad, and observe_chain has no autograd"):
            mod.observe_chain(a, *va, x, cs)
        with pytest.raises(TaylorError, match="degree_p1 = 1"):  # the shape rules come first
            mod.observe_chain(a, *va, x, cs, degree_p1=1)
        with torch.no_grad():
            with pytest.raises(TaylorError, match="on cpu"):
                mod.observe_chain(a, *va, x, cs)


# ---- the host argument layer ----------------------------------------------------------------------------------------------------


def test_series_args_on_observation_chains(tmp_path):
    """tests/series_observe_chain_args_main.cpp: a plain host program over gft_series_args.hpp -- the same refusals in C with their
    texts and order, the strides of x and cs in the collapsed batch, the overlaps; under AddressSanitizer and
    UndefinedBehaviorSanitizer where the compiler has them and the program runs with them"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "obc_args")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "genfer_amd", "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "series_observe_chain_args_main.cpp")]
    for extra in (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []):
        if subprocess.run(base + extra, capture_output=True).returncode != 0:
            continue
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        if extra and out.returncode != 0 and "FAILED" not in out.stdout:
            continue  # (the sanitizers' runtime does not start here: the plain build decides)
        assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
        m = re.search(r"^ok (\d+) checks$", out.stdout.strip().splitlines()[-1])
        assert m and int(m.group(1)) >= 40, out.stdout
        return
    pytest.fail("tests/series_observe_chain_args_main.cpp does not build")


# ---- the kernels' code ------------------------------------------------------------------------------------------------------------


def test_series_observe_chain_isa(tmp_path):
    """The gfx950 code of the four kernels (two forms per element type): no scratch, no calls, no f64 FMA and no division; form A
    allocates no LDS and exchanges values between lanes (ds_bpermute_b32), form B has no static LDS either (its two line buffers are
    dynamic) and goes through ds reads and writes around a barrier."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", "series_observe_chain_isa_check.hip")],
                          cwd=tmp_path)
    isa = open(glob.glob(str(tmp_path / "*amdgcn-amd-amdhsa*gfx950*.s"))[0]).read()
    assert isa.count(".private_segment_fixed_size: 0") == 4 and isa.count(".private_segment_fixed_size:") == 4
    assert isa.count(".amdhsa_group_segment_fixed_size 0\n") == 4
    assert isa.count(".vgpr_spill_count: 0") == 4
    kernels = {}
    for m in re.finditer(r"^(_ZN3gft\w+):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M):
        kernels[m.group(1)] = [ln.split()[0] for ln in m.group(2).splitlines() if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((".", ";"))]
    assert len(kernels) == 4
    for name, code in kernels.items():
        assert len(code) > 30, name
        assert not [c for c in code if c.startswith(("scratch_", "buffer_", "flat_"))], name
        assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")], name
        assert not [c for c in code if ("fma" in c and "f64" in c) or c.startswith("v_div_")], name
        assert any(c.startswith("global_load") for c in code) and any(c.startswith("global_store") for c in code), name
        assert any(c.startswith("v_mul_f64") for c in code) and any(c.startswith("v_add_f64") for c in code), name
        lds = [c for c in code if c.startswith("ds_") and "permute" not in c]
        if "k_obs_chain_wave" in name:
            assert not lds and "s_barrier" not in code, name
            assert any(c.startswith("ds_bpermute_b32") for c in code), name
        else:
            assert any(c.startswith("ds_read") for c in lds) and any(c.startswith("ds_write") for c in lds) and "s_barrier" in code, name
