"""The batched observation ops (derivative, taylor_expansion_of_coeff, shift_down, evaluate_all_one of genfer_amd.series, series2,
interval_series, interval_series2 and series2_grad; gft_series_* / gft_series2_* and their gfti_ twins) without a GPU: the numpy
model of tests/_series_observe_model.py against the oracle's handle API bit for bit (the GPU tests use the model where the batch
is large), the exported surface, every refusal made before a device is touched, the adjoint identities of the backward passes, and
the gfx950 code of the kernels."""
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _series_observe_model as M
from _series2_oracle import bits_equal
from conftest import ROOT, splitmix64_uniform

OPS = ("derivative", "taylor_expansion_of_coeff", "shift_down", "evaluate_all_one")
SYMBOLS = tuple(f"{pre}{rank}_{op}" for pre in ("gft_", "gfti_") for rank in ("series", "series2") for op in OPS)
LENGTHS = (1, 2, 7, 8, 9, 17)
SHAPES = ((1, 6), (6, 1), (9, 1), (17, 1), (3, 5), (8, 8), (4, 17), (12, 7), (2, 33))
B = 2  # items per model call: the model is vectorised over them, the oracle takes one at a time


def orders(length):
    return sorted({k for k in (0, 1, 7, 8, 9, length - 1) if 0 <= k < length})


def data(kind, shape, seed, interval=False):
    """dense: 0.5 + uniform; mixed: uniform - 0.5 (mixed signs); no exact zeros.  Intervals: [v, v + a small positive width]"""
    n = int(np.prod(shape))
    u = splitmix64_uniform(seed, n).reshape(shape)
    v = 0.5 + u if kind == "dense" else u - 0.5
    assert (v != 0.0).all()
    if not interval:
        return v
    w = splitmix64_uniform(seed + 77, n).reshape(shape) * 1e-3
    hi = v + w
    assert (hi != 0.0).all()
    return np.stack([v, hi])


def oracle_item(T, op, item, shape, var, k):
    return getattr(T.new(item, shape), op)(var, k).array()


def check(got, want, what):
    ok = bits_equal(got, want)
    assert ok.all(), f"{what}: {(~ok).sum()} coefficients differ, first at {tuple(np.argwhere(~ok)[0])}"


# ---- the model against the oracle ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["dense", "mixed"])
@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("n", LENGTHS)
def test_model_is_the_oracle_at_rank_1(OTP, OTPI, n, interval, kind):
    T, A = (OTPI, M.IV) if interval else (OTP, M.F64)
    x = data(kind, (B, n), 100 + n, interval)
    for op in OPS[:3]:
        for k in orders(n):
            got = getattr(M, op)(A, x, -1, k) if op != "shift_down" else M.shift_down(A, x, -1, k, 1)
            for b in range(B):
                check(got[:, b] if interval else got[b], oracle_item(T, op, x[:, b] if interval else x[b], (n,), 0, k), f"{op} n={n} k={k} item {b}")


@pytest.mark.parametrize("kind", ["dense", "mixed"])
@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_is_the_oracle_at_rank_2(OTP, OTPI, shape, interval, kind):
    T, A = (OTPI, M.IV) if interval else (OTP, M.F64)
    x = data(kind, (B,) + shape, 200 + 40 * shape[0] + shape[1], interval)
    for op in OPS[:3]:
        for var in (0, 1):
            for k in orders(shape[var]):
                got = getattr(M, op)(A, x, var - 2, k) if op != "shift_down" else M.shift_down(A, x, var - 2, k, 2)
                for b in range(B):
                    check(got[:, b] if interval else got[b], oracle_item(T, op, x[:, b] if interval else x[b], shape, var, k),
                          f"{op} {shape} var={var} k={k} item {b}")


@pytest.mark.parametrize("shape", [(n,) for n in LENGTHS] + list(SHAPES), ids=str)
def test_evaluate_all_one_model_is_the_plain_fold(oracle_lib, shape):
    """the oracle's handle API has no entry for it: the definition is the fold of mt:583-586, 0.0 + x[0] + x[1] + ... in row-major order"""
    from _series2_interval_model import Ops

    rank = len(shape)
    for kind in ("dense", "mixed"):
        x = data(kind, (B,) + shape, 300 + sum(shape))
        got = M.evaluate_all_one(M.F64, x, rank)
        for b in range(B):
            acc = 0.0
            for v in x[b].reshape(-1):
                acc = acc + float(v)
            assert bits_equal(got[b], np.float64(acc)).all()
        xi = data(kind, (B,) + shape, 300 + sum(shape), True)
        goti = M.evaluate_all_one(M.IV, xi, rank)
        o = Ops(oracle_lib)
        for b in range(B):
            acc = (0.0, 0.0)
            for lo, hi in zip(xi[0, b].reshape(-1), xi[1, b].reshape(-1)):
                acc = o.add(acc, (lo, hi))
            assert bits_equal(goti[:, b], np.array(acc)).all()


def test_negative_zero_at_k_0(OTP):
    """the additions of 0.0 are real: shift_down(k = 0) turns coefficient 0 = -0.0 into +0.0 and leaves the other -0.0 alone; the
    scalings keep the sign; evaluate_all_one of an all -0.0 item is +0.0"""
    x = np.array([[-0.0, 1.5, -0.0, 2.0]])
    for rank, item, shape, var in ((1, x[0], (4,), 0), (2, x, (1, 4), 1), (2, x.T.copy(), (4, 1), 0)):
        arr = item[None]
        got = M.shift_down(M.F64, arr, (var - 2) if rank == 2 else -1, 0, rank)[0]
        want = oracle_item(OTP, "shift_down", item, shape, var, 0)
        check(got, want, f"shift_down rank {rank}")
        assert not np.signbit(got.reshape(-1)[0]) and np.signbit(got.reshape(-1)[2])
        for op in ("derivative", "taylor_expansion_of_coeff"):
            got = getattr(M, op)(M.F64, arr, (var - 2) if rank == 2 else -1, 0)[0]
            check(got, oracle_item(OTP, op, item, shape, var, 0), op)
            assert np.signbit(got.reshape(-1)[0])
    ev = M.evaluate_all_one(M.F64, np.full((1, 3), -0.0), 1)
    assert ev[0] == 0.0 and not np.signbit(ev[0])


def test_factors_are_not_the_integers_one_would_guess():
    """ff_{j+1} = ff_j * ((k + j + 1) / (j + 1)) rounds the quotient first: the table differs from the exact falling factorials"""
    fs = np.array(M.factors(M.F64, "derivative", 3, 40))
    exact = np.array([float(np.prod([float(j + i) for i in range(1, 4)])) for j in range(40)])
    assert fs[0] == 6.0 and (fs != exact).any()
    assert np.allclose(fs, exact, rtol=1e-13)


# ---- the adjoint identities ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape,axis", [((6,), -1), ((5, 4), -1), ((5, 4), -2), ((7, 1), -2), ((1, 7), -1)], ids=str)
def test_adjoint_identities_in_integers(shape, axis):
    """<op(x), g> = <x, op^T(g)> exactly on small integers; the orders are those whose factors are integers, so nothing rounds"""
    rng = np.random.default_rng(11 + sum(shape))
    rank, ln = len(shape), shape[axis]
    x = rng.integers(-3, 4, size=(2,) + shape).astype(np.float64)
    for op in ("derivative", "coeff"):
        for k in range(ln):
            fs = M.factors(M.F64, op, k, ln - k)
            if not all(float(f).is_integer() for f in fs):
                continue
            y = M._scaled(M.F64, op, x, axis, k)
            g = rng.integers(-3, 4, size=y.shape).astype(np.float64)
            gx = M.scaled_adj(op, g, axis, k)
            assert gx.shape == x.shape and float((y * g).sum()) == float((x * gx).sum())
            assert not np.signbit(np.moveaxis(gx, axis, -1)[..., :k]).any()  # +0.0 below k
    for k in range(ln):
        y = M.shift_down(M.F64, x, axis, k, rank)
        g = rng.integers(-3, 4, size=y.shape).astype(np.float64)
        gx = M.shift_down_adj(g, axis, k)
        assert gx.shape == x.shape and float((y * g).sum()) == float((x * gx).sum())
    y = M.evaluate_all_one(M.F64, x, rank)
    g = rng.integers(-3, 4, size=y.shape).astype(np.float64)
    assert float((y * g).sum()) == float((x * M.evaluate_all_one_adj(g, shape)).sum())


# ---- the surface ------------------------------------------------------------------------------------------------------------------


def test_symbols_are_declared_and_exported():
    """4 operations x 2 ranks x 2 element types = 16 entry points, and the 20 Python functions over them"""
    import genfer_amd

    if not os.path.exists(genfer_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    L = genfer_amd.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len(SYMBOLS) == 16
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert hasattr(L, s), s
        assert f"pub fn {s}(" in doc, s
    from genfer_amd import interval_series, interval_series2, series, series2, series2_grad

    for mod in (series, series2, interval_series, interval_series2, series2_grad):
        for op in OPS:
            assert callable(getattr(mod, op)), (mod.__name__, op)
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_extern.py"), "--check"])


def test_modules_import_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "from genfer_amd import series, series2, interval_series, interval_series2, series2_grad\n"
            "assert callable(series.derivative) and callable(series2_grad.shift_down) and callable(interval_series2.evaluate_all_one)\nprint('ok')")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_bench_series_observe_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_series_observe.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "--shapes" in out.stdout and "--rounds" in out.stdout


# ---- refusals that need no device -------------------------------------------------------------------------------------------------


def modules():
    from genfer_amd import interval_series, interval_series2, series, series2, series2_grad

    return {"series": (series, 1, 0), "series2": (series2, 2, 0), "interval_series": (interval_series, 1, 1),
            "interval_series2": (interval_series2, 2, 1), "series2_grad": (series2_grad, 2, 0)}


@pytest.mark.parametrize("name", ["series", "series2", "interval_series", "interval_series2", "series2_grad"])
def test_refusals_need_no_device(name):
    torch = pytest.importorskip("torch")
    from genfer_amd.taylor import TaylorError

    mod, rank, planes = modules()[name]
    lead = (2,) * planes
    item = (6,) if rank == 1 else (4, 6)
    x = torch.ones(lead + (3,) + item, dtype=torch.float64)
    va = (1,) if rank == 2 else ()  # var
    raw = "series2" if name == "series2_grad" else name  # with nothing tracked series2_grad's calls are series2's
    for op in OPS[:3]:
        f = getattr(mod, op)
        for k in (6, 7, -1):
            with pytest.raises(TaylorError, match=rf"{raw}\.{op}: k = {k}, but x has 6 stored coefficients"):
                f(x, *va, k)
        with pytest.raises(TypeError, match="non-negative integer"):
            f(x, *va, 1.5)
        with pytest.raises(TypeError, match="non-negative integer"):
            f(x, *va, True)
        if rank == 2:
            with pytest.raises(TaylorError, match=r"k = 4, but x has 4 stored coefficients on axis -2"):
                f(x, 0, 4)
            for var in (2, -1, True, None, 0.0):
                with pytest.raises(TaylorError, match="is 0 .* or 1"):
                    f(x, var, 1)
            with pytest.raises(TaylorError, match="at least"):
                f(x[(0,) * planes + (0, 0)] if not planes else x[:, 0, 0], 1, 1)
            with pytest.raises(TaylorError, match="is empty"):
                f(x[..., :0, :], 1, 1)
        else:
            with pytest.raises(TaylorError, match="is empty"):
                f(x[..., :0], 0)
        with pytest.raises(TaylorError, match="unit stride"):
            f(x[..., ::2], *va, 1)
        with pytest.raises(TaylorError, match="float32"):
            f(x.float(), *va, 1)
        with pytest.raises(TypeError, match="torch.Tensor"):
            f([[1.0]], *va, 0)
        with pytest.raises(TaylorError, match="out has shape"):  # the result is k shorter on the axis
            f(x, *va, 2, out=torch.empty(lead + (3,) + item, dtype=torch.float64))
        with pytest.raises(TaylorError, match="out has batch shape"):
            f(x, *va, 2, out=torch.empty(lead + (2,) + item[:-1] + (4,), dtype=torch.float64))
        with pytest.raises(TaylorError, match="on cpu"):  # everything else in order: the placement is judged last
            f(x, *va, 2)
    ev = mod.evaluate_all_one
    with pytest.raises(TaylorError, match="out has batch shape"):
        ev(x, out=torch.empty(lead + (4,), dtype=torch.float64))
    with pytest.raises(TaylorError, match="out has batch shape"):  # the result has no series axis
        ev(x, out=torch.empty(lead + (3,) + item, dtype=torch.float64))
    with pytest.raises(TaylorError, match="float32"):
        ev(x.float())
    with pytest.raises(TaylorError, match="on cpu"):
        ev(x)
    with pytest.raises(TaylorError, match="on cpu"):
        ev(x, out=torch.empty(lead + (3,), dtype=torch.float64))
    limit = {"series": 4096, "series2": 4096, "series2_grad": 4096, "interval_series": 2048, "interval_series2": 2048}[name]
    big = torch.ones(lead + ((limit + 1,) if rank == 1 else (limit // 64 + 1, 64)), dtype=torch.float64)
    for op in OPS:
        args = () if op == "evaluate_all_one" else va + (1,)
        with pytest.raises(TaylorError, match=f"exceeds the limit of {limit}"):
            getattr(mod, op)(big, *args)
    at = torch.ones(lead + ((limit,) if rank == 1 else (limit // 64, 64)), dtype=torch.float64)
    with pytest.raises(TaylorError, match="on cpu"):  # the limit itself passes
        mod.evaluate_all_one(at)


@pytest.mark.parametrize("name", ["series", "series2", "interval_series", "interval_series2", "series2_grad"])
def test_tracked_operands_without_a_device(name):
    """series and series2_grad differentiate (and refuse out= with a tracked operand); series2 and the interval modules refuse a
    tracked operand with series2's wording"""
    torch = pytest.importorskip("torch")
    from genfer_amd.taylor import TaylorError

    mod, rank, planes = modules()[name]
    lead = (2,) * planes
    item = (6,) if rank == 1 else (4, 6)
    xg = torch.ones(lead + (3,) + item, dtype=torch.float64, requires_grad=True)
    va = (1,) if rank == 2 else ()
    for op in OPS:
        args = () if op == "evaluate_all_one" else va + (2,)
        f = getattr(mod, op)
        if name in ("series", "series2_grad"):
            with pytest.raises(TaylorError, match="out= cannot be combined with an operand that requires grad"):
                f(xg, *args, out=torch.empty(3, dtype=torch.float64))
            with pytest.raises(TaylorError, match=f"{name}.{op}: .*on cpu"):
                f(xg, *args)
            if op != "evaluate_all_one":
                with pytest.raises(TaylorError, match="k = 6, but x has 6"):
                    f(xg, *va, 6)
        else:
            with pytest.raises(TaylorError, match=f"this version of {name} has no autograd"):
                f(xg, *args)
        with torch.no_grad():
            with pytest.raises(TaylorError, match="on cpu"):
                f(xg, *args)


# ---- the kernels' code ------------------------------------------------------------------------------------------------------------


def test_series_observe_isa(tmp_path):
    """The gfx950 code of the ten kernels (tests/series_observe_isa_check.hip: five per element type): no scratch, no buffer
    instructions, no calls, and no f64 FMA of any kind -- the only division sequence of the feature is the factor table's, which is
    k_factor_table's and not in these kernels; the scalings multiply (v_mul_f64), the sums add (v_add_f64), and the row kernels
    exchange values between lanes without LDS allocation."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", "series_observe_isa_check.hip")],
                          cwd=tmp_path)
    isa = open(glob.glob(str(tmp_path / "*amdgcn-amd-amdhsa*gfx950*.s"))[0]).read()
    assert isa.count(".private_segment_fixed_size: 0") == 10 and isa.count(".private_segment_fixed_size:") == 10
    assert isa.count(".amdhsa_group_segment_fixed_size 0\n") == 10
    kernels = {}
    for m in re.finditer(r"^(_ZN3gft\w+):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M):
        kernels[m.group(1)] = [ln.split()[0] for ln in m.group(2).splitlines() if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((".", ";"))]
    assert len(kernels) == 10
    for name, code in kernels.items():
        assert len(code) > 30, name
        assert not [c for c in code if c.startswith("scratch_") or c.startswith("buffer_")], name
        assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")], name
        # (the f32 FMAs of the index divisions, v_fmac_f32 behind v_rcp_iflag_f32, touch no coefficient)
        assert not [c for c in code if ("fma" in c and "f64" in c) or c.startswith("v_div_")], name
        assert any(c.startswith("global_load") for c in code) and any(c.startswith("global_store") for c in code), name
        if "k_obs_scale" in name:
            assert any(c.startswith("v_mul_f64") for c in code), name
        else:
            assert any(c.startswith("v_add_f64") for c in code), name
