"""compose and pow of the batched trivariate series (genfer_amd.series3, gft_series3_compose / gft_series3_pow) without a GPU: the
chains of series3.mul's products that define them against the CPU oracle's own subst_var / pow and against the plain-Python model,
the two sentinels of the squeeze, the stand-alone program of the HIP-free planner, the declared surface and the refusals the
Python side makes before it touches a device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _series3_compose_cases as cc
import make_series_refusals as table
from _series3_oracle import bits_equal, dense
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
INF, NAN = float("inf"), float("nan")


def test_chains_against_the_oracle(OTP, oracle_lib):
    """0 differing bits, signs of zeros included, on dense and signed data: the oracle is normative there"""
    composed = powered = 0
    for n in cc.ORACLE_SHAPES:
        for var, fs, gs, kind in cc.oracle_compose_cases(n):
            f, g = cc.make(kind, fs, 17 * n[0] + n[2] + var), cc.make(kind, gs, 31 * n[1] + n[2] + var + 5)
            ok = bits_equal(cc.chain_compose(oracle_lib, f, g, var, n), cc.oracle_compose(OTP, f, g, var, n))
            assert ok.all(), ("compose", n, var, fs, gs, kind)
            composed += 1
        for xs, kind, e in cc.oracle_pow_cases(n):
            x = cc.make(kind, xs, 13 * n[0] + n[1] + e)
            assert bits_equal(cc.chain_pow(oracle_lib, x, e, n), cc.oracle_pow(OTP, x, e, n)).all(), ("pow", n, xs, kind, e)
            powered += 1
    assert (composed, powered) == (576, 252)


def specials(shape, seed):
    """an item with infinities, a NaN and zeros of both signs among plain coefficients"""
    a = dense(shape, seed).reshape(-1)
    for i, v in enumerate([INF, -0.0, NAN, 0.0, -INF, -0.0]):
        a[(3 + 5 * i) % a.size] = v
    return a.reshape(shape)


def test_chains_against_the_model(oracle_lib):
    """small items, the products in plain Python: special values, a constant g, a one-slice f, unit axes"""
    checked = 0
    with np.errstate(all="ignore"):
        for n in [(2, 2, 2), (3, 2, 3), (2, 3, 1), (1, 3, 3), (1, 1, 4)]:
            for var in (0, 1, 2):
                one = tuple(1 if a == var else n[a] for a in range(3))
                for fs, gs in [(n, n), (n, (1, 1, 1)), (one, n), (n, tuple(min(2, v) for v in n))]:
                    for f, g in [(dense(fs, 5), dense(gs, 6)), (specials(fs, 7), dense(gs, 8)), (dense(fs, 9), specials(gs, 10)),
                                 (-np.abs(specials(fs, 11)), specials(gs, 12))]:
                        ok = bits_equal(cc.chain_compose(oracle_lib, f, g, var, n), cc.model_compose(f, g, var, n))
                        assert ok.all(), ("compose", n, var, fs, gs)
                        checked += 1
            for e in cc.POW_E:
                for x in (dense(n, 13), specials(n, 14), -np.abs(specials(cc.compact_shapes(n)[0], 15))):
                    assert bits_equal(cc.chain_pow(oracle_lib, x, e, n), cc.model_pow(x, e, n)).all(), ("pow", n, e)
                    checked += 1
    assert checked == 5 * 3 * 4 * 4 + 5 * 7 * 3
    # a one-slice f: 0.0 + f, g's values not read (a g of NaNs changes nothing); -0.0 becomes +0.0
    f = dense((1, 2, 3), 16)
    f[0, 1, 1] = -0.0
    got = cc.chain_compose(oracle_lib, f, np.full((2, 2, 2), NAN), 0, (2, 2, 3))
    assert bits_equal(got, cc.pad3(0.0 + f, (2, 2, 3))).all() and not np.signbit(got).any()
    # pow: e = 1 runs the loop (-0.0 becomes +0.0), e = 0 is the unit item
    x = dense((2, 2, 2), 17)
    x[1, 0, 1] = -0.0
    got = cc.chain_pow(oracle_lib, x, 1, (2, 2, 2))
    assert bits_equal(got, 0.0 + x).all() and not np.signbit(got).any()
    unit = np.zeros((2, 3, 2))
    unit[0, 0, 0] = 1.0
    assert bits_equal(cc.chain_pow(oracle_lib, specials((2, 2, 2), 18), 0, (2, 3, 2)), unit).all()


def test_the_squeeze_is_part_of_the_definition(oracle_lib):
    """the two sentinels: every product in the caller's axis order WITHOUT the squeeze (one accumulator over (j0, j1)) differs from
    the chain -- measured: 3 (dense) and 9 (signed) of 40 coefficients, 4 and 9 of 64"""
    counts = []
    for fs, gs, n, var in cc.SENTINELS:
        for kind in ("dense", "signed"):
            f, g = cc.make(kind, fs, 3), cc.make(kind, gs, 4)
            chain = cc.chain_compose(oracle_lib, f, g, var, n)
            assert bits_equal(chain, cc.model_compose(f, g, var, n)).all()
            off = ~bits_equal(cc.unsqueezed_compose(f, g, var, n), chain)
            assert off.any(), (fs, gs, n, var, kind)
            counts.append((int(off.sum()), int(np.prod(n))))
    assert counts == [(3, 40), (9, 40), (4, 64), (9, 64)]


def test_step_shapes_keep_their_unit_axes():
    """the invariance the planner relies on, over every small shape: the unit axes of every step are those of the last"""
    import itertools

    shapes = list(itertools.product((1, 2, 3), repeat=3))
    checked = 0
    for n in shapes:
        fit = [s for s in shapes if all(s[a] <= n[a] for a in range(3))]
        for nf in fit:
            for ng in fit:
                for var in (0, 1, 2):
                    steps = cc.step_shapes(nf, ng, n, var)
                    for s in steps[1:]:
                        assert [v == 1 for v in s] == [v == 1 for v in steps[-1]], (nf, ng, n, var, steps)
                    checked += 1
    assert checked == 3 * (1 + 4 + 9) ** 3  # per n: (n0 * n1 * n2)^2 pairs of shapes that fit, three variables


def test_planner_program_builds_and_passes(tmp_path):
    """tests/series3_compose_args_main.cpp: the step shapes, the one permutation and the refusal texts of the HIP-free argument layer,
    under AddressSanitizer and UndefinedBehaviorSanitizer where the compiler has them and the program runs with them"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "series3_compose_args_main")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "series3_compose_args_main.cpp")]
    for extra in (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []):
        if subprocess.run(base + extra, capture_output=True).returncode != 0:
            continue
        done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        if extra and done.returncode != 0 and "FAILED" not in done.stdout:
            continue  # (the sanitizers' runtime does not start here: the plain build decides)
        assert done.returncode == 0 and done.stdout.startswith("OK checks="), (done.returncode, done.stdout[-3000:], done.stderr[-3000:])
        assert int(done.stdout.split("checks=")[1].split()[0]) > 100000
        return
    pytest.fail("tests/series3_compose_args_main.cpp does not build")


def test_symbols_are_declared_and_exported():
    import re

    import genfer_amd

    if not os.path.exists(genfer_amd.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    L = genfer_amd.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gftaylor.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in ("gft_series3_compose", "gft_series3_pow"):
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert hasattr(L, s), s
        assert f"pub fn {s}(" in doc, s
    from genfer_amd import _series_call, series3

    assert callable(series3.compose) and callable(series3.pow)
    assert _series_call.RANK3 == ("mul", "div", "exp", "log", "compose", "pow")
    # the declarations come from the one table: var behind the operands, e behind x
    import ctypes as C

    lib = _series_call._lib()
    comp, pw = lib.gft_series3_compose.argtypes, lib.gft_series3_pow.argtypes
    assert len(comp) == 25 and comp[14] is C.c_int and len(pw) == 18 and pw[7] is C.c_uint32


def test_python_side_refusals_need_no_device():
    """storage-less tensors that report a GPU placement reach every check in front of the library"""
    torch = pytest.importorskip("torch")
    from genfer_amd import series2, series3
    from genfer_amd.taylor import TaylorError

    def T(*shape, **kw):
        return table._tensor(torch, dict({"t": list(shape)}, **kw))

    f, g = T(3, 2, 4, 8), T(3, 2, 4, 8)
    for var in (3, -1, True, 1.0):
        with pytest.raises(TaylorError, match=r"series3\.compose: var = .*0 \(axis -3\), 1 \(axis -2\) or 2 \(axis -1\)"):
            series3.compose(f, g, var=var)
    with pytest.raises(TaylorError, match=r"series2\.compose: var = 2; the variable of f that g replaces is 0 or 1"):  # (unchanged)
        series2.compose(T(3, 4, 8), T(3, 4, 8), var=2)
    with pytest.raises(TypeError, match="got a bool"):
        series3.pow(f, True)
    with pytest.raises(TypeError, match="non-integral"):
        series3.pow(f, 2.5)
    with pytest.raises(TaylorError, match=r"series3\.pow: e = -1 is negative \(use series3\.div"):
        series3.pow(f, -1)
    with pytest.raises(TaylorError, match="does not fit the 32 bits"):
        series3.pow(f, 2**32)
    for call in (lambda *a, **k: series3.compose(f, *a, **k), lambda *a, **k: series3.compose(*a, g, **k),
                 lambda *a, **k: series3.pow(*(a or (f,)), 3, **k)):
        for n in [(1, 4, 8), (2, 3, 8), (2, 4, 7)]:  # an operand longer than n, on each axis
            with pytest.raises(TaylorError, match="nx > n"):
                call(f, n=n)
        with pytest.raises(TaylorError, match=r"n0 \* n1 \* n2 = 17 \* 241 \* 1 = 4097 exceeds the limit of 4096"):
            call(T(3, 1, 1, 1), n=(17, 241, 1))
        with pytest.raises(TaylorError, match=r"out has \(2, 4, 9\)"):
            call(f, out=T(3, 2, 4, 9))
        with pytest.raises(TaylorError, match="batch shape"):
            call(f, out=T(1, 2, 4, 8))
        with pytest.raises(TaylorError, match="no autograd"):
            call(T(3, 2, 4, 8, grad=True))
        with pytest.raises(TaylorError, match="float32"):
            call(T(3, 2, 4, 8, dtype="float32"))
        with pytest.raises(TaylorError, match="at least 3"):
            call(T(4, 8))
        with pytest.raises(TaylorError, match="on cpu"):  # everything else in order: the placement is judged last
            call(T(3, 2, 4, 8, on="cpu"))
    with pytest.raises(TaylorError, match=r"series3\.compose: out has"):
        series3.compose(f, g, var=2, out=T(3, 2, 4, 9))
