"""The transposed product series.corr (gft_series_corr) and the transposed Horner loop series._compose_adj (gft_series_compose_adj)
on the MI355X.  Every coefficient of every item carries the bits of the definition: the reference's product orc_mul_raw on the
flipped row (tests/test_series_corr_cpu.py shows that this is the written-out descending loop).  Both forms of corr and the
planner's own choice; views, a result in place, refusals."""
import ctypes as C

import numpy as np
import pytest

from test_series_compose_cpu import dense
from test_series_corr_cpu import want_compose_adj, want_corr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 0x5A5A5A5A5A5A5A5A
ORDERS = [1, 2, 3, 7, 31, 32, 33, 63, 64, 65, 79, 80, 100, 257, 1024, 4096]
BATCHES = [1, 3, 64, 65, 1000]
CPU_BUDGET = 7.0e7  # B * n^2 per case, as in test_series_batch_gpu.py
A_MAX_N, A_MAX_N_PLAIN = 79, 63  # the largest ng of form A with 80 KB / 64 KB of LDS a workgroup (mul's budget)
SA_MIN_ITEMS = 256


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


def assert_bits(got, want, what):
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    ok = np.where(nan, np.isnan(got), got.view(np.int64) == want.view(np.int64))
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {(~ok).sum()} coefficients differ, first at {i}: got {got[i]!r} want {want[i]!r}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def compact_cases(ng):
    """(ny, m) out of ny in {1, ng // 3, ng - 1} x m in {1, ng // 2, ng - 1}, where they are lengths"""
    out = []
    for ny in (1, ng // 3, ng - 1):
        for m in (1, ng // 2, ng - 1):
            if 1 <= ny <= ng and 1 <= m <= ng and (ny, m) != (ng, ng) and (ny, m) not in out:
                out.append((ny, m))
    return out


def corr_cases(ng):
    """(B, ny, m): dense on every batch size the budget allows, the compact lengths on two of them"""
    for B in BATCHES:
        if B * ng * ng > CPU_BUDGET:
            continue
        yield B, ng, ng
        if B in (3, 65) or (ng >= 1024 and B == 1):
            for ny, m in compact_cases(ng):
                yield B, ny, m


@pytest.mark.parametrize("ng", ORDERS)
def test_corr_bit_exact_against_the_flipped_product(ng, oracle_lib):
    from genfer_amd import series

    seen = set()
    for B, ny, m in corr_cases(ng):
        g, y = dense((B, ng), 1000 * ng + 17 * B + ny), dense((B, ny), 3000 * ng + 13 * B + m + 5)
        want = want_corr(oracle_lib, g, y, m)  # once per case, for the three runs
        G, Y = dev(g), dev(y)
        for form in (None, "A", "B"):
            series.set_form(form)
            got = series.corr(G, Y, m)
            ran = series.last_form()
            assert_bits(got, want, f"corr ng={ng} B={B} ny={ny} m={m} asked {form} ran {ran}")
            if form == "B" or ng > A_MAX_N:
                assert ran == "B", (ng, B, form, ran)
            elif form == "A" and ng <= A_MAX_N_PLAIN:
                assert ran == "A", (ng, B, form, ran)
            elif form is None and ng <= A_MAX_N_PLAIN:
                assert ran == ("A" if B >= SA_MIN_ITEMS else "B"), (ng, B, ran)  # mul's dispatch
            else:
                assert ran in ("A", "B")
            seen.add(ran)
        series.set_form(None)
    assert "B" in seen and (ng > A_MAX_N or "A" in seen)


def test_default_m_and_special_values(oracle_lib):
    from genfer_amd import series

    inf, nan = float("inf"), float("nan")
    g = np.array([[1.0, 2.0, inf, 4.0, 5.0], [0.0, -0.0, 1.0, nan, 2.0], [1.0, 0.0, 0.0, 0.0, inf], [-0.0] * 5])
    y = np.array([[3.0, 0.5], [1.0, inf], [0.0, 1.0], [-0.0, 0.0]])
    want = want_corr(oracle_lib, g, y, 5)
    for form in ("A", "B"):
        series.set_form(form)
        got = series.corr(dev(g), dev(y))  # m defaults to ng
        assert series.last_form() == form
        assert_bits(got, want, f"corr specials, form {form}")
    # the outputs a compact y does not carry the infinity to stay finite: no term from padding
    assert np.isfinite(want[0][[0, 3, 4]]).all()


@pytest.mark.parametrize("ng,batch", [(12, (5, 70)), (40, (3, 4, 6)), (130, (2, 5))])
def test_views_and_in_place(ng, batch, oracle_lib):
    from genfer_amd import series

    B = int(np.prod(batch))
    ny, m = max(1, ng // 2), ng - 1
    g, y = dense((B, ng), 21), dense((B, ny), 22)
    want = want_corr(oracle_lib, g, y, m).reshape(batch + (m,))
    G, Y = dev(g).reshape(batch + (ng,)), dev(y).reshape(batch + (ny,))
    # y at batch stride 0, as an expanded view and as a 1-d tensor
    w0 = want_corr(oracle_lib, g, np.repeat(y[:1], B, axis=0), m).reshape(batch + (m,))
    ye = dev(y[:1]).reshape((1,) * len(batch) + (ny,)).expand(batch + (ny,))
    assert ye.stride()[0] == 0
    assert_bits(series.corr(G, ye, m), w0, "expanded y")
    assert_bits(series.corr(G, dev(y[0]), m), w0, "1-d y")
    # a strided batch view of g
    wide = torch.zeros(batch[:-1] + (2 * batch[-1], ng + 7), dtype=torch.float64, device=DEV)
    wide[..., ::2, 3:3 + ng] = G
    gs = wide[..., ::2, 3:3 + ng]
    assert not gs.is_contiguous() and gs.stride(-1) == 1
    assert_bits(series.corr(gs, Y, m), want, "strided g")
    # a strided out with guard words around it
    for form in ("A", "B"):
        series.set_form(form)
        big = torch.full(batch + (m + 5,), GUARD, dtype=torch.int64, device=DEV).view(torch.float64)
        out = big[..., 2:2 + m]
        assert series.corr(gs, Y, m, out=out) is out
        assert_bits(out, want, f"sliced out, form {form}")
        gw = big.view(torch.int64)
        assert bool((gw[..., :2] == GUARD).all()) and bool((gw[..., 2 + m:] == GUARD).all())
        # in place on g (m == ng: the same view)
        gi = G.clone()
        assert series.corr(gi, Y, out=gi) is gi
        assert_bits(gi, want_corr(oracle_lib, g, y, ng).reshape(batch + (ng,)), f"corr in place on g, form {form}")
    series.set_form(None)


def test_in_place_on_one_long_series(oracle_lib):
    """a result in place may not be spread over workgroups: one series long enough for several"""
    from genfer_amd import series

    g, y = dense((2, 700), 31), dense((2, 700), 32)
    gi = dev(g)
    series.corr(gi, dev(y), out=gi)
    assert series.last_form() == "B"
    assert_bits(gi, want_corr(oracle_lib, g, y, 700), "corr in place, 700 coefficients")


def test_refusals():
    from genfer_amd import series
    from genfer_amd.taylor import TaylorError
    import genfer_amd

    g = torch.rand((6, 16), dtype=torch.float64, device=DEV)
    y = torch.rand((6, 16), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="m = 17 > 16"):
        series.corr(g, y, 17)
    with pytest.raises(TaylorError, match="y has 17 coefficients"):
        series.corr(g, torch.rand((6, 17), dtype=torch.float64, device=DEV))
    with pytest.raises(TaylorError, match="4096"):
        series.corr(torch.rand((1, 4097), dtype=torch.float64, device=DEV), y)
    buf = torch.rand((6, 40), dtype=torch.float64, device=DEV)
    with pytest.raises(TaylorError, match="partially overlaps g"):
        series.corr(buf[:, 0:16], y, out=buf[:, 8:24])
    with pytest.raises(TaylorError, match="partially overlaps y"):
        series.corr(g, buf[:, 0:16], out=buf[:, 8:24])
    with pytest.raises(TaylorError, match="overlaps y"):  # not even as the same view
        yi = y.clone()
        series.corr(g, yi, out=yi)
    with pytest.raises(TaylorError, match="overlaps g"):  # compose_adj's result is never the inner series
        gi = y.clone()
        series._compose_adj(g, gi, 16, out=gi)
    # through the C entry points
    series.last_form()  # declares them
    L = genfer_amd.lib()
    one = (C.c_size_t * 1)(6)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = torch.empty((6, 16), dtype=torch.float64, device=DEV)
    assert L.gft_series_corr(vp(g), None, 8, vp(y), None, 8, vp(out), None, 9, one, 1, None) == -1
    assert "m = 9 > ng = 8" in L.gft_last_error().decode()
    assert L.gft_series_corr(vp(g), None, 8, vp(y), None, 9, vp(out), None, 8, one, 1, None) == -1
    assert "ny = 9 > ng = 8" in L.gft_last_error().decode()
    assert L.gft_series_corr(vp(g), None, 4097, vp(y), None, 8, vp(out), None, 8, one, 1, None) == -1
    assert "4096" in L.gft_last_error().decode()
    assert L.gft_series_corr(vp(g), None, 8, vp(y), None, 8, vp(out), None, 0, one, 1, None) == -1
    assert "m == 0" in L.gft_last_error().decode()
    assert L.gft_series_compose_adj(vp(g), None, 8, vp(y), None, 8, vp(out), None, 9, one, 1, None) == -1
    assert "nf = 9 > n = 8" in L.gft_last_error().decode()
    assert L.gft_series_compose_adj(vp(g), None, 8, vp(y), None, 9, vp(out), None, 8, one, 1, None) == -1
    assert "ng = 9 > n = 8" in L.gft_last_error().decode()
    z = torch.zeros((0, 8), dtype=torch.float64, device=DEV)
    assert series.corr(z, z).shape == (0, 8) and series._compose_adj(z, z, 3).shape == (0, 3)
    assert float((g + 1.0).sum().item()) > 0  # no stale HIP error


ADJ_CASES = [(1, 1, 1, 1), (5, 1, 8, 1), (4, 2, 9, 1), (7, 3, 7, 1), (16, 16, 16, 1), (64, 33, 65, 1), (3, 100, 257, 1), (16, 4096, 4096, 1),
             (64, 64, 64, 300)]  # (nf, ng, n, B): compact lengths growing by 0, by 1, and hitting the cap early


@pytest.mark.parametrize("nf,ng,n,B", ADJ_CASES)
def test_compose_adj_bit_exact_against_the_chain(nf, ng, n, B, oracle_lib):
    from genfer_amd import series

    gh, g = dense((B, n), 50 * n + nf), dense((B, ng), 60 * n + ng)
    want = want_compose_adj(oracle_lib, gh, g, nf)
    GH, G = dev(gh), dev(g)
    got = series._compose_adj(GH, G, nf)
    assert series.last_form() == "B"  # its one form
    assert got.shape == (B, nf)
    assert_bits(got, want, f"compose_adj nf={nf} ng={ng} n={n} B={B}")
    # the chain of public calls on the device carries the same bits
    ls = [min(1 + (nf - 1 - i) * (ng - 1), n) for i in range(nf)]
    a = GH[:, :ls[0]]
    outs = [a[:, 0]]
    for i in range(nf - 1):
        a = series.corr(a, G[:, :min(ng, a.shape[-1])], ls[i + 1])
        outs.append(a[:, 0])
    assert torch.equal(torch.stack(outs, dim=-1).view(torch.int64), got.view(torch.int64))
    if nf == n:  # in place on gh
        gi = GH.clone()
        assert series._compose_adj(gi, G, nf, out=gi) is gi
        assert_bits(gi, want, "compose_adj in place on gh")
    # one inner series for a whole batch
    if B > 1:
        w0 = want_compose_adj(oracle_lib, gh, np.repeat(g[:1], B, axis=0), nf)
        assert_bits(series._compose_adj(GH, G[0], nf), w0, "compose_adj, 1-d g")
