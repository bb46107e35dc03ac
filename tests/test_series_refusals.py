"""The refusals of the batched series layer, whole messages: tests/series_refusals.json (written by tests/make_series_refusals.py
from the commit before the host layers were folded into one descriptor and one runner) replayed against this tree.

  * the Python layer, on the CPU: storage-less tensors that report a GPU placement reach every check in front of the library;
  * the C layer, on the GPU: raw calls of the entry points, torch's next operation succeeding behind every refusal;
  * the C layer again without a device: tests/series_args_main.cpp, a stand-alone program around the HIP-free
    genfer_amd/csrc/gft_series_args.hpp, built with the host compiler, must give the same messages -- and, for a handful of
    accepted calls, the collapsed batch that was reviewed once and is pinned in the table.
"""
import os
import shutil
import subprocess

import pytest

import make_series_refusals as table

HERE = os.path.dirname(os.path.abspath(__file__))
T = table.load()


def test_table_covers_the_generators_cases():
    """the committed table is the generator's current case list, in order (a case added there must be recorded)"""
    assert [e["case"] for e in T["c"]] == table.c_cases()
    assert [e["case"] for e in T["accepted"]] == table.accepted_cases()
    assert [e["case"] for e in T["python"]] == table.python_cases()
    assert len(T["c"]) >= 120 and all(e["message"] for e in T["c"] if 0 not in (e["case"]["batch"] or []))


def test_python_layer_messages():
    got = table.record_python()
    assert len(got) == len(T["python"]) > 0
    for g, want in zip(got, T["python"]):
        assert (g["type"], g["message"]) == (want["type"], want["message"]), want["case"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("series_args") / "series_args_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "series_args_main.cpp")])
    return exe


def test_c_layer_messages_without_a_device(program):
    entries = [e for e in T["c"] if not e["case"].get("device_only")]
    lines = table.run_program(program, [e["case"] for e in entries])
    for e, line in zip(entries, lines):
        assert line == ("EMPTY" if e["message"] is None else "E " + e["message"]), e["case"]


def test_accepted_calls_collapse_as_recorded(program):
    lines = table.run_program(program, [e["case"] for e in T["accepted"]])
    assert lines == [e["plan"] for e in T["accepted"]]
    assert sum(line.startswith("OK ") for line in lines) >= 5


def test_the_two_operation_tables_agree(program):
    """gft::SERIES_OPS (the program's "ops" mode) and _series_call.OPS, row by row in the enum's order: as many operations, the same
    long side, the same name of the first operand, the same operations at rank 3"""
    from genfer_amd import _series_call

    rows = [line.split(" ", 4) for line in subprocess.check_output([program, "ops"], text=True).splitlines()]
    ops = list(_series_call.OPS.values())
    assert len(rows) == len(ops) and [int(r[0]) for r in rows] == list(range(len(ops)))
    assert [o.suffix for o in ops][:len(table.OPS)] == table.OPS  # (the generator states an op by its position in the enum)
    for (_, _family, ranks, long, names), o in zip(rows, ops):
        assert long == o.long, o.suffix
        assert names.split("|")[0] == o.names[0], o.suffix
        assert (int(ranks) == 3) == (o.suffix in _series_call.RANK3), o.suffix
        assert int(ranks) in (2, 3), o.suffix


@pytest.mark.gpu
def test_c_layer_messages_on_the_gpu():
    checked = []

    def after(buf):  # no stale HIP error: torch's next call succeeds
        checked.append(float((buf[:16] + 1.0).sum().item()))

    for (c, rc, msg), e in zip(table.replay_c([e["case"] for e in T["c"]], after), T["c"]):
        assert (rc, msg) == ((0, None) if e["message"] is None else (-1, e["message"])), c
    assert checked == [16.0] * len(T["c"])
