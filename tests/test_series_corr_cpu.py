"""The transposed product corr and the transposed Horner loop compose_adj (genfer_amd.series.corr / _compose_adj, gft_series_corr /
gft_series_compose_adj) without a GPU: the definition -- the written-out descending loop against orc_mul_raw on the flipped row,
which is where the GPU tests take their expected values from (tests/test_series_corr_gpu.py imports the shims of this file) --
the gfx950 code of the three kernels, the exported surface and the refusals the Python side makes before it touches the library."""
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_series_compose_cpu import _device_like, dense, mul_raw, same_bits

SYMBOLS = ("gft_series_corr", "gft_series_compose_adj")
INF, NAN = float("inf"), float("nan")

# ---- the expected values shared with the GPU tests ---------------------------------------------------------------------------


def corr_ref(oracle_lib, g, y, m=None):
    """corr(g, y)[:m] from the reference's product: mul_1d(flip(g), y) truncated at ng, read backwards"""
    g, y = np.asarray(g, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ng = g.size
    m = ng if m is None else m
    assert y.size <= ng and 1 <= m <= ng
    with np.errstate(all="ignore"):
        z = mul_raw(oracle_lib, np.ascontiguousarray(g[::-1]), y, ng)
    return np.ascontiguousarray(z[::-1][:m])


def adj_lengths(nf, ng, n):
    return [min(1 + (nf - 1 - i) * (ng - 1), n) for i in range(nf)]


def compose_adj_ref(oracle_lib, gh, g, nf):
    """the chain: a_0 = gh[:l_0], out[i] = a_i[0], a_{i+1} = corr(a_i, g, l_{i+1})"""
    gh, g = np.asarray(gh, dtype=np.float64), np.asarray(g, dtype=np.float64)
    ls = adj_lengths(nf, g.size, gh.size)
    a = gh[:ls[0]].copy()
    out = [a[0]]
    for i in range(nf - 1):
        a = corr_ref(oracle_lib, a, g[:min(g.size, a.size)], ls[i + 1])  # (coefficients of g beyond the row meet no term)
        out.append(a[0])
    return np.array(out, dtype=np.float64)


def want_corr(oracle_lib, G, Y, m):
    return np.stack([corr_ref(oracle_lib, G[b], Y[b], m) for b in range(G.shape[0])])


def want_compose_adj(oracle_lib, GH, G, nf):
    return np.stack([compose_adj_ref(oracle_lib, GH[b], G[b], nf) for b in range(GH.shape[0])])


# ---- the definition --------------------------------------------------------------------------------------------------------------


def corr_loops(g, y, m):
    """section 1 of the definition, written out: descending k, a sum from +0, only stored operands"""
    ng, ny = len(g), len(y)
    out = np.zeros(m)
    with np.errstate(all="ignore"):
        for i in range(m):
            s = np.float64(0.0)
            for k in range(min(ng - 1, i + ny - 1), i - 1, -1):
                s = s + np.float64(g[k]) * np.float64(y[k - i])
            out[i] = s
    return out


def corr_cases(ng):
    """(ny, m): dense, and the compact corners ny < ng, ny = 1, m < ng"""
    cand = [(ng, ng), (ng - 1, ng), (1, ng), (ng, 1), (ng // 3, ng // 2), (ng - 1, ng - 1), (ng // 2, ng)]
    out = []
    for ny, m in cand:
        if 1 <= ny <= ng and 1 <= m <= ng and (ny, m) not in out:
            out.append((ny, m))
    return out


@pytest.mark.parametrize("ng", [1, 2, 3, 7, 33, 100])
def test_the_written_loop_is_the_flipped_product(ng, oracle_lib):
    for ny, m in corr_cases(ng):
        g, y = dense((ng,), 40 * ng + ny), dense((ny,), 41 * ng + m)
        rows = [(g, y)]
        for v in (0.0, -0.0, INF, NAN):  # a special value in g, in y, at the ends and inside
            for pos in {0, ng // 2, ng - 1}:
                gs = g.copy()
                gs[pos] = v
                rows.append((gs, y))
            for pos in {0, ny // 2, ny - 1}:
                ys = y.copy()
                ys[pos] = v
                rows.append((g, ys))
        gs = g.copy()
        gs[ng - 1] = INF
        ys = y.copy()
        ys[0] = 0.0  # inf * 0: a NaN exactly where the two meet
        rows.append((gs, ys))
        for gr, yr in rows:
            assert same_bits(corr_ref(oracle_lib, gr, yr, m), corr_loops(gr, yr, m)), (ng, ny, m)


def test_no_term_is_formed_from_padding(oracle_lib):
    """a compact y beside an infinity in g: a padded zero would turn the outputs it does not reach into NaN"""
    g = np.array([1.0, 2.0, INF, 4.0, 5.0])
    c = corr_ref(oracle_lib, g, np.array([3.0, 0.5]), 5)
    assert same_bits(c, np.array([4.0, INF, INF, 14.5, 15.0]))
    assert same_bits(c, corr_loops(g, [3.0, 0.5], 5))


def test_adjoint_identity_in_integers(oracle_lib):
    """<mul(x, y), g> = <x, corr(g, y)> exactly on small integers, compact operands included"""
    rng = np.random.default_rng(5)
    for nx, ny, n in [(6, 6, 6), (3, 6, 6), (6, 2, 6), (4, 3, 5), (1, 1, 1), (5, 5, 9)]:
        x, y, g = (rng.integers(-3, 4, size=k).astype(np.float64) for k in (nx, ny, n))
        z = mul_raw(oracle_lib, x, y, n)
        assert float(np.dot(z, g)) == float(np.dot(x, corr_ref(oracle_lib, g, y, nx))), (nx, ny, n)


def compose_adj_loops(gh, g, nf):
    n, ng = len(gh), len(g)
    ls = adj_lengths(nf, ng, n)
    a = [np.float64(v) for v in gh[:ls[0]]]
    out = [a[0]]
    with np.errstate(all="ignore"):
        for i in range(nf - 1):
            new = []
            for p in range(ls[i + 1]):
                s = np.float64(0.0)
                for k in range(min(ls[i] - 1, p + ng - 1), p - 1, -1):
                    s = s + a[k] * np.float64(g[k - p])
                new.append(s)
            a = new
            out.append(a[0])
    return np.array(out, dtype=np.float64)


ADJ_CASES = [(1, 1, 1), (5, 1, 8), (4, 2, 9), (7, 3, 7), (16, 16, 16), (3, 5, 4), (6, 4, 30), (1, 3, 5), (9, 2, 5)]  # (nf, ng, n)


def test_compose_adj_chain_is_the_written_loops(oracle_lib):
    for nf, ng, n in ADJ_CASES:
        gh, g = dense((n,), 7 * n + nf), dense((ng,), 9 * n + ng)
        assert same_bits(compose_adj_ref(oracle_lib, gh, g, nf), compose_adj_loops(gh, g, nf)), (nf, ng, n)
        gs = gh.copy()
        gs[n // 2] = INF
        g0 = g.copy()
        g0[ng - 1] = 0.0
        assert same_bits(compose_adj_ref(oracle_lib, gs, g0, nf), compose_adj_loops(gs, g0, nf)), (nf, ng, n)


def test_compose_adj_is_the_gradient_of_compose_in_integers(oracle_lib):
    """out[i] = <gh, g^i truncated at n> exactly on small integers (dh/df_i = g^i)"""
    from test_series_compose_cpu import chain_pow

    rng = np.random.default_rng(11)
    for nf, ng, n in [(4, 3, 6), (5, 2, 4), (3, 4, 9), (1, 2, 3)]:
        gh, g = rng.integers(-3, 4, size=n).astype(np.float64), rng.integers(-2, 3, size=ng).astype(np.float64)
        want = [float(np.dot(gh, chain_pow(oracle_lib, g, i, n))) for i in range(nf)]
        assert compose_adj_ref(oracle_lib, gh, g, nf).tolist() == want, (nf, ng, n)


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
    assert "DESCENDING" in open(os.path.join(ROOT, "include", "gftaylor.h")).read()  # the order of the sums is stated


def test_module_surface():
    from genfer_amd import series

    assert callable(series.corr) and callable(series._compose_adj)
    assert "descending" in series.corr.__doc__
    assert "requires_grad" in series.__doc__


def test_python_side_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError

    x = torch.zeros((3, 8), dtype=torch.float64)
    d = _device_like(torch, (3, 8))
    with pytest.raises(TaylorError, match="g: .*on cpu"):
        series.corr(x, x)
    with pytest.raises(TaylorError, match="y: .*on cpu"):
        series.corr(d, x)
    with pytest.raises(TaylorError, match="g: .*float32"):
        series.corr(x.float(), x)
    with pytest.raises(TaylorError, match="y: .*float32"):
        series.corr(d, _device_like(torch, (3, 8)).float())
    with pytest.raises(TypeError, match="g: .*torch.Tensor"):
        series.corr([1.0, 2.0], x)
    with pytest.raises(TypeError, match="y: .*torch.Tensor"):
        series.corr(d, [1.0, 2.0])
    with pytest.raises(TaylorError, match="g: .*unit stride"):
        series.corr(_device_like(torch, (3, 16))[:, ::2], d)
    with pytest.raises(TaylorError, match="y: .*unit stride"):
        series.corr(d, _device_like(torch, (3, 16))[:, ::2])
    with pytest.raises(TaylorError, match="m = 9 > 8.*of g"):
        series.corr(d, d, m=9)
    with pytest.raises(TaylorError, match="y has 9 coefficients, more than the 8 of g"):
        series.corr(d, _device_like(torch, (3, 9)))
    with pytest.raises(TaylorError, match="m = 0"):
        series.corr(d, d, m=0)
    with pytest.raises(TaylorError, match="g has 4097 coefficients.*4096"):
        series.corr(_device_like(torch, (1, 4097)), d)
    with pytest.raises(TaylorError, match="gh: .*on cpu"):
        series._compose_adj(x, x, 3)
    with pytest.raises(TaylorError, match="nf = 9 > 8.*of gh"):
        series._compose_adj(d, d, 9)


def test_bench_series_knows_the_new_legs():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_series", os.path.join(ROOT, "tools", "bench_series.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["--ops", "corr,backward"]).ops == "corr,backward"
    assert "corr" in mod.KNOWN_OPS and "backward" in mod.KNOWN_OPS


# ---- the gfx950 code ---------------------------------------------------------------------------------------------------------------


def test_corr_isa(tmp_path):
    """The gfx950 code of corr form A, corr form B and compose_adj (tests/series_corr_isa_check.hip): no scratch, no calls, LDS
    reads, separately rounded v_mul_f64 / v_add_f64 and no v_fma_f64 (nor a contracted multiply-add of another spelling)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"), os.path.join(ROOT, "tests", "series_corr_isa_check.hip")],
                          cwd=tmp_path)
    isa = open(glob.glob(str(tmp_path / "*amdgcn-amd-amdhsa*gfx950*.s"))[0]).read()
    assert isa.count(".private_segment_fixed_size: 0") == 3 and isa.count(".private_segment_fixed_size:") == 3
    kernels = {}
    name = None
    for line in isa.splitlines():
        m = re.match(r"^(_ZN3gft\w+):", line)
        if m:
            name = m.group(1)
            kernels[name] = []
        elif line.startswith("\t.end_amdhsa_kernel") or line.startswith("\t.section"):
            name = None
        elif name and line.startswith("\t") and not line.lstrip().startswith("."):
            kernels[name].append(line.split()[0])
    found = {key: [c for k, c in kernels.items() if key in k] for key in ("k_series_corr_a", "k_series_corr_b", "k_series_compose_adj_b")}
    for key, codes in found.items():
        assert len(codes) == 1 and len(codes[0]) > 50, key
        code = codes[0]
        assert not [c for c in code if c.startswith("scratch_")], key
        assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")], key
        assert any(c.startswith("ds_read") or c.startswith("ds_load") for c in code), key
        assert any(c.startswith("v_mul_f64") for c in code) and any(c.startswith("v_add_f64") for c in code), key
        assert not [c for c in code if "fma" in c or c.startswith("v_fmac") or c.startswith("v_mad_f64")], key + ": a contracted multiply-add"
    assert any(c == "s_barrier" for c in found["k_series_compose_adj_b"][0])  # the steps meet at a barrier
