"""The generator of tests/_graph_programs.py against the oracle alone: what its programs must contain for the GPU replays
(tests/test_graph_programs_gpu.py) to mean something, and that a schedule — when values are read, when handles are released —
never changes a value on the reference."""
import numpy as np
import pytest

import _graph_programs as gp

SEEDS = range(1, 41)
N_INSTR = 40
_CACHE = {}


def _program(T, seed):
    key = (T.WIDTH, seed)
    if key not in _CACHE:
        prog = gp.generate(T, seed, N_INSTR)
        _CACHE[key] = (prog, gp.replay(T, prog, "straight"))
    return _CACHE[key]


@pytest.fixture(params=["f64", "interval"])
def O(request, OTP, OTPI):
    return OTPI if request.param == "interval" else OTP


@pytest.mark.parametrize("seed", SEEDS)
def test_programs_hold_what_the_gpu_replays_rely_on(seed, O):
    prog, straight = _program(O, seed)  # (the oracle rejected nothing: generate() and replay() do not catch its errors)
    assert len(prog["instrs"]) == gp.N_LEAVES + N_INSTR
    assert sum(len(i["outs"]) for i in prog["instrs"]) == len(prog["handles"]) == len(straight)
    for (h, reader), vals in straight.items():
        shape, deg, arr = vals[0]
        assert shape == prog["handles"][h]["shape"] and deg == prog["handles"][h]["deg"]
        assert np.all(np.isfinite(arr)), (h, prog["instrs"])
        # above the host tier of the default dispatch: the product records it
        assert int(np.prod(shape)) > gp.SIZE_FLOOR, (h, shape)
    kinds = {i["kind"] for i in prog["instrs"]} - {"leaf"}
    assert len(kinds) >= 9, sorted(set(gp.KINDS) - kinds)
    shared = [h for h, use in gp.consumers(prog).items() if len(use) >= 2]
    assert len(shared) >= 15, len(shared)
    acts = gp.plan(prog, "drops")
    first_read = next(k for k, a in enumerate(acts) if a[0] == "read")
    released = [a[1] for a in acts[:first_read] if a[0] == "release"]
    assert len(released) >= 5 and len(set(released)) == len(released)
    assert not any(a[0] == "release" for a in acts[first_read:])
    read = {a[1] for a in acts if a[0] == "read"}
    assert read.isdisjoint(released) and read | set(released) == set(range(len(prog["handles"])))
    # released while recordings still read them (not sinks), and sinks nobody ever reads
    use = gp.consumers(prog)
    assert any(use[h] for h in released)


@pytest.mark.parametrize("seed", SEEDS)
def test_a_schedule_does_not_change_values_on_the_reference(seed, O):
    prog, straight = _program(O, seed)
    for schedule in gp.SCHEDULES:
        got = gp.replay(O, prog, schedule)
        assert got, schedule
        acts = gp.plan(prog, schedule)
        for (h, reader), vals in got.items():
            shape, deg, arr = straight[(h, "array")][0]
            indices = [a[3] for a in acts if a[:3] == ("read", h, reader)]  # (in reading order, as the values)
            assert len(indices) == len(vals)
            for idx, val in zip(indices, vals):
                if reader in ("array", "clone_array"):
                    want = (shape, deg, arr)
                elif reader == "constant_term":
                    want = np.atleast_1d(arr[(Ellipsis,) + (0,) * len(shape)])
                elif reader == "coefficient":
                    want = np.atleast_1d(arr[(Ellipsis,) + idx])
                else:
                    want = bool(np.all(arr == 0.0))
                assert gp.same_value(want, val), (schedule, h, reader)
                if reader in ("array", "clone_array"):
                    assert np.array_equal(arr.view(np.uint64), val[2].view(np.uint64)), (schedule, h, reader)


def test_schedules_cover_what_they_are_for():
    """The plans themselves (no backend): every schedule reads every handle it keeps, `interleaved` reads in the middle with
    every reader over the seed set, `grow` records on top of a half-read program."""
    readers, mid_reads = set(), 0
    for seed in SEEDS:
        # (a program skeleton is enough for plan(): shapes and use lists)
        rng_prog = {"seed": seed, "handles": [{"shape": (50, 50), "deg": (50, 50)}] * 43,
                    "instrs": [{"kind": "leaf", "ins": [], "outs": [k]} for k in range(3)] +
                              [{"kind": "scale", "ins": [k - 1], "outs": [k]} for k in range(3, 43)]}
        for schedule in ("last_first", "as_created", "interleaved", "grow"):
            acts = gp.plan(rng_prog, schedule)
            assert {a[1] for a in acts if a[0] == "read"} == set(range(43)), schedule
            assert [a[1] for a in acts if a[0] == "exec"] == list(range(43)), schedule
        acts = gp.plan(rng_prog, "interleaved")
        last_exec = max(k for k, a in enumerate(acts) if a[0] == "exec")
        mid = [a for a in acts[:last_exec] if a[0] == "read"]
        mid_reads += len(mid)
        readers |= {a[2] for a in mid}
        acts = gp.plan(rng_prog, "grow")
        kinds = [a[0] for a in acts]
        first_read = kinds.index("read")
        assert "exec" in kinds[first_read:], "grow: nothing recorded after the first reads"
    assert readers == set(gp.READERS), readers
    assert mid_reads >= len(SEEDS)
