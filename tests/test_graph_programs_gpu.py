"""Random shared-handle programs (tests/_graph_programs.py) replayed through the deferred launch graph.

The programs are plain data, pinned against the oracle alone by tests/test_graph_programs_cpu.py; here they are only REPLAYED
on the product — under five schedules of reading and releasing, with the graph on and off — and every value read must be the
oracle's, bit for bit.  What the hand-built ladders of test_horner_shapes_gpu.py and the interpreter's own programs do not
reach: recordings with several consumers on different levels, handles freed while a recording still reads them, recordings
nobody reads, values read in the middle of a program, and levels wide enough to split a batch group, to exceed a segment
of the argument arena and to wrap its ring."""
import os

import numpy as np
import pytest

import _graph_programs as gp
from conftest import splitmix64_uniform

pytestmark = pytest.mark.gpu

SEEDS = range(1, 13)
N_INSTR = 40
# the switches under which the verification matrix runs the suite: bits only then (the gate of test_horner_shapes_gpu.py)
SWITCHES = ("GFT_BATCH", "GFT_LAZY_OBSERVE", "GFT_LAZY_HORNER", "GFT_LAZY_SUM", "GFT_NZ_PROOFS", "GFT_DEFER", "GFT_HORNER_LOOP_MAX")
_ORACLE = {}


def _case(O, seed):
    """The program of (element type, seed) and the oracle's reads under every schedule: computed once, shared, never changed."""
    key = (O.WIDTH, seed)
    if key not in _ORACLE:
        prog = gp.generate(O, seed, N_INSTR)
        _ORACLE[key] = (prog, {s: gp.replay(O, prog, s) for s in gp.SCHEDULES})
    return _ORACLE[key]


def _classes(interval, OTP, GTP, OTPI, GTPI):
    return (OTPI, GTPI) if interval else (OTP, GTP)


class _batch_dag:
    """`batch_dag` = on for the block, the default (1) afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import genfer_amd

        self.L = genfer_amd.lib()
        assert self.L.gft_set_option(b"batch_dag", float(self.on)) == 0

    def __exit__(self, *exc):
        self.L.gft_set_option(b"batch_dag", 1.0)


def _delta(before):
    import genfer_amd

    after = genfer_amd.op_stats()
    return {k: after[k] - before[k] for k in after}


# ---- A: random programs, every schedule, graph on and off --------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["device", "host"], indirect=True)
@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("seed", SEEDS)
def test_random_programs_bit_exact_under_every_schedule(seed, interval, tier, OTP, GTP, OTPI, GTPI):
    O, G = _classes(interval, OTP, GTP, OTPI, GTPI)
    prog, want = _case(O, seed)
    for batch in (1, 0):
        with _batch_dag(batch):
            for schedule in gp.SCHEDULES:
                got = gp.replay(G, prog, schedule)  # (a call that raises fails the test)
                gp.assert_same_reads(want[schedule], got, f"seed {seed} {schedule} batch_dag={batch} tier={tier}")


# ---- B: the graph was taken -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["host"], indirect=True)
@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_programs_run_through_the_graph(interval, tier, OTP, GTP, OTPI, GTPI):
    """Under the default dispatch the programs' idioms ARE recordings: summed over the seed set, one `last_first` replay each
    (the first read executes the deepest graph), the counters show graph executions, batches of several items, nested Adds,
    observation chains with an Add as epilogue and recorded materialisations; with the graph off no batch is launched."""
    import genfer_amd

    O, G = _classes(interval, OTP, GTP, OTPI, GTPI)
    switched = any(os.environ.get(k) for k in SWITCHES)
    total = {}
    for batch in (1, 0):
        with _batch_dag(batch):
            before = genfer_amd.op_stats()
            for seed in SEEDS:
                prog, want = _case(O, seed)
                gp.assert_same_reads(want["last_first"], gp.replay(G, prog, "last_first"), f"seed {seed} batch_dag={batch}")
            total[batch] = _delta(before)
    print(total)
    if switched:  # (the verification matrix: values only)
        return
    d = total[1]
    assert d["graph_executions"] > 0 and d["graph_recordings"] > 0, d
    assert d["batch_items"] > d["batch_launches"] > 0, d
    assert d["nested_adds"] > 0, d
    assert d["fused_observe_adds"] > 0, d
    assert d["chains_materialised"] > 0, d
    assert total[0]["batch_launches"] == 0, total[0]


# ---- C: released handles give their memory back ---------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["device", "host"], indirect=True)
@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("seed", [2, 5, 11])
def test_released_handles_return_their_memory(seed, interval, tier, OTP, GTP, OTPI, GTPI):
    """A replay that releases every handle — some of them while recordings still read them, some recordings never read —
    leaves the pool where it was."""
    import genfer_amd

    L = genfer_amd.lib()
    O, G = _classes(interval, OTP, GTP, OTPI, GTPI)
    prog, want = _case(O, seed)
    for batch in (1, 0):
        with _batch_dag(batch):
            for schedule in ("drops", "last_first"):
                # Warm what is bounded by design and outlives the handles: the kernels' grow-only workspaces, the cache of
                # derivative-factor tables and the cache of power tables (Ops::pow_table: at most 257 scalings, then emptied —
                # a warm-up that crosses that bound re-forms its tables in the second one).
                for _ in range(2):
                    gp.replay(G, prog, schedule)
                assert L.gft_synchronize() == 0
                before = genfer_amd.pool_stats()["in_use"]
                got = gp.replay(G, prog, schedule)
                assert L.gft_synchronize() == 0
                after = genfer_amd.pool_stats()["in_use"]
                gp.assert_same_reads(want[schedule], got, f"seed {seed} {schedule} batch_dag={batch}")
                assert after == before, (schedule, batch, before, after)


# ---- D: wide levels ---------------------------------------------------------------------------------------------------------
# The sizes below come from sizeof(ObsItem) = 1456 bytes, ArgArena::SEG = 8 MB, NSEG = 8 and the group cap of SEG / 2
# (gft_batch.hpp batch_alloc): a group holds at most 2880 items, a segment 5761, the ring 46 091.  If the item struct shrinks,
# the launch-count assertions below fail: that is the signal to raise M until a level splits / exceeds a segment again.
WIDE_N = 16


def _wide_leaf(seed, width):
    base = (0.05 + 0.95 * splitmix64_uniform(seed, WIDE_N * WIDE_N)).reshape(WIDE_N, WIDE_N)
    return np.stack([base, base * (1 + 1e-15)]) if width == 2 else base


def _wide_level(T, M, seed):
    """M independent two-step observation chains on one leaf, distinct x, all recorded before any read — and ONE value that
    depends on all of them (their running sum at one degree less: the truncated views keep the Adds from taking a chain as
    their own epilogue, so the M chains are one level of plain recordings).  Returns (items, root)."""
    n = WIDE_N
    sc = (lambda v: (v, v)) if T.WIDTH == 2 else (lambda v: v)
    arr = _wide_leaf(seed, T.WIDTH)
    g = T.new(arr, [n, n])
    root = T.new(np.ascontiguousarray(arr[..., : n - 3, : n - 3]), [n - 3, n - 3])
    items = []
    for i in range(M):
        a = g.observe_chain(i % 2, sc(0.05 + 0.9 * i / M), [sc(0.1), sc(0.05)], n - 2)
        items.append(a)
        root = root + a
    return items, root


def _same(o, g):
    return o.degrees_p1() == g.degrees_p1() and o.coeffs_shape() == g.coeffs_shape() and gp.same_floats(o.array(), g.array())


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
@pytest.mark.parametrize("M,min_launches", [(3000, 2), (6000, 3)], ids=["splits_a_group", "exceeds_a_segment"])
def test_wide_level_splits_its_batch(M, min_launches, interval, OTP, GTP, OTPI, GTPI):
    """3000 items of one geometry are more than a group takes (2880): two launches, one upload.  6000 are more than a segment
    of the arena (5761): the level goes up in several pieces (batch_flush).  Every item carries the oracle's bits."""
    import genfer_amd

    O, G = _classes(interval, OTP, GTP, OTPI, GTPI)
    want_items, want_root = _wide_level(O, M, 900 + M)
    before = genfer_amd.op_stats()
    items, root = _wide_level(G, M, 900 + M)
    recorded = _delta(before)
    assert _same(want_root, root)  # the first read: one graph execution, the M chains its first level
    d = _delta(before)
    bad = [i for i in range(M) if not _same(want_items[i], items[i])]
    assert not bad, (len(bad), bad[:8])
    if any(os.environ.get(k) for k in SWITCHES):
        return
    assert recorded["batch_launches"] == 0 and recorded["graph_executions"] == 0, recorded  # nothing ran before the read
    assert d["batch_items"] == M, d
    assert d["batch_launches"] >= min_launches, d
    assert _delta(before)["graph_executions"] == d["graph_executions"], "reading an item executed a graph: it was not in memory"


@pytest.mark.parametrize("interval", [False, True], ids=["f64", "interval"])
def test_wide_levels_wrap_the_argument_ring(interval, OTP, GTP, OTPI, GTPI):
    """Nine rounds of 6000 items with fresh data: 54 000 items against 46 091 for the ring of 8 segments, so segments are
    written again behind the events of the launches that read them.  Every item of every round is compared."""
    import genfer_amd

    O, G = _classes(interval, OTP, GTP, OTPI, GTPI)
    M = 6000
    before = genfer_amd.op_stats()
    for rnd in range(9):
        want_items, want_root = _wide_level(O, M, 2000 + rnd)
        items, root = _wide_level(G, M, 2000 + rnd)
        assert _same(want_root, root), rnd
        bad = [i for i in range(M) if not _same(want_items[i], items[i])]
        assert not bad, (rnd, len(bad), bad[:8])
        del items, root, want_items, want_root
    d = _delta(before)
    if not any(os.environ.get(k) for k in SWITCHES):
        assert d["batch_items"] == 9 * M and d["batch_launches"] >= 27, d
