"""The rank-3 refusals of the HIP-free argument layer (genfer_amd/csrc/gft_series_args.hpp) and a few accepted calls, without a
device: tests/series3_args_main.cpp, a stand-alone program built with the host compiler -- under AddressSanitizer and
UndefinedBehaviorSanitizer where the compiler has them and the program runs with them.  The accepted calls pin the collapsed
batch, the stored result shape S and the permuted item the kernels run (reviewed by eye against gft_series_args.hpp's rules)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MUL, DIV, EXP, LOG = 0, 1, 2, 3


def V(off, shape, sst=None, rst=None, bs=None):
    """a view: `off` doubles into the buffer (None: a null pointer), contiguous unless the strides say otherwise"""
    s0, s1, s2 = shape
    return {"off": off, "bs": bs, "sst": s1 * s2 if sst is None else sst, "rst": s2 if rst is None else rst, "shape": shape}


SEED, NOSEED = {"off": 4000, "bs": None, "sst": 0, "rst": 0, "shape": (1, 1, 1)}, {"off": None, "bs": None, "sst": 0, "rst": 0, "shape": (1, 1, 1)}
N = (2, 3, 4)
X, Y, R = V(0, N), V(100, N), V(200, N)

REFUSED = [
    ((MUL, [3], X, Y, V(200, (2, 0, 4))), "series3_mul: n0 * n1 * n2 == 0 (the result has no coefficients)"),
    ((MUL, [3], X, Y, V(200, (17, 241, 1))), "series3_mul: n0 * n1 * n2 = 17 * 241 * 1 exceeds the limit of 4096 coefficients per item of this version"),
    ((DIV, [3], X, Y, V(200, (4097, 1, 1))), "series3_div: n0 * n1 * n2 = 4097 * 1 * 1 exceeds the limit of 4096 coefficients per item of this version"),
    ((MUL, [3], V(0, (0, 3, 4)), Y, R), "series3_mul: an operand has no coefficients"),
    ((DIV, [3], X, V(100, (2, 3, 0)), R), "series3_div: an operand has no coefficients"),
    ((MUL, [3], V(0, (3, 3, 4)), Y, R), "series3_mul: x has 3 x 3 x 4 coefficients, the result 2 x 3 x 4 (an operand is longer than the truncation order)"),
    ((DIV, [3], X, V(100, (2, 4, 4)), R), "series3_div: y has 2 x 4 x 4 coefficients, the result 2 x 3 x 4 (an operand is longer than the truncation order)"),
    ((EXP, [3], V(0, (2, 3, 5)), SEED, R), "series3_exp: x has 2 x 3 x 5 coefficients, the result 2 x 3 x 4 (an operand is longer than the truncation order)"),
    ((LOG, [2] * 33, X, NOSEED, R), "series3_log: more than 32 batch axes"),
    ((MUL, None, X, Y, R), "series3_mul: the batch shape is a null pointer"),
    ((MUL, [1 << 16, 1 << 15], X, Y, R), "series3_mul: more than 2^31 - 1 series in one call"),
    ((MUL, [3], V(0, N, sst=-12), Y, R), "series3_mul: negative strides are not supported (x, the slab axis)"),
    ((MUL, [3], X, V(100, N, rst=-4), R), "series3_mul: negative strides are not supported (y, the row axis)"),
    ((MUL, [3], X, Y, V(200, N, bs=[-24])), "series3_mul: negative strides are not supported (the result, batch axis 0)"),
    ((MUL, [3], X, Y, V(200, N, bs=[0])), "series3_mul: the result has a zero stride (batch axis 0): its series overlap"),
    ((MUL, [3], X, Y, V(200, N, sst=0)), "series3_mul: the result has a zero slab stride: the slabs of an item overlap"),
    ((MUL, [3], X, Y, V(200, N, rst=0)), "series3_mul: the result has a zero row stride: the rows of an item overlap"),
    ((MUL, [3], X, Y, V(200, N, sst=8)), "series3_mul: the result's series overlap each other (its strides do not separate the rows)"),
    ((MUL, [3], X, Y, V(200, N, bs=[12])), "series3_mul: the result's series overlap each other (its strides do not separate the rows)"),
    ((MUL, [3], X, Y, V(4, N)), "series3_mul: the result partially overlaps x (it may alias an operand only as the same view)"),
    ((DIV, [3], X, Y, V(100, N, sst=16, bs=[40])), "series3_div: the result partially overlaps y (it may alias an operand only as the same view)"),
    ((EXP, [3], X, {"off": 210, "bs": None, "sst": 0, "rst": 0, "shape": (1, 1, 1)}, R),
     "series3_exp: the result partially overlaps the seeds (it may alias an operand only as the same view)"),
]

# accepted: what the call collapses to, then S, the permuted item (`run`, the operands' shapes and the strides of its three axes)
ACCEPTED = [
    # contiguous, full shapes: one merged batch axis, nothing permuted
    ((MUL, [3, 4], X, V(1000, N), V(2000, N)),
     "OK nd=1 items=12 inplace=0 ext=[12] xs=[24] ys=[24] ss=[0] rs=[24] rows=4,4,4 slabs=12,12,12 | S=[2,3,4] run=[2,3,4] x=[2,3,4] y=[2,3,4] "
     "xst=[12,4,1] yst=[12,4,1] rst=[12,4,1]"),
    # in place on x, through slab and row strides of a wider tensor
    ((DIV, [3], V(0, N, sst=40, rst=10, bs=[100]), V(1000, N), V(0, N, sst=40, rst=10, bs=[100])),
     "OK nd=1 items=3 inplace=1 ext=[3] xs=[100] ys=[24] ss=[0] rs=[100] rows=10,4,10 slabs=40,12,40 | S=[2,3,4] run=[2,3,4] x=[2,3,4] y=[2,3,4] "
     "xst=[40,10,1] yst=[12,4,1] rst=[40,10,1]"),
    # exp of x stored as (4, 2, 1) at (5, 3, 2): S = (5, 3, 1) runs as the rank-2 item (1, 5, 3), the row stride innermost
    ((EXP, [3], V(0, (4, 2, 1)), SEED, V(200, (5, 3, 2))),
     "OK nd=1 items=3 inplace=0 ext=[3] xs=[8] ys=[0] ss=[1] rs=[30] rows=1,0,2 slabs=2,0,6 | S=[5,3,1] run=[1,5,3] x=[1,4,2] y=[1,1,1] "
     "xst=[1,2,1] yst=[0,0,0] rst=[1,6,2]"),
    # mul of two thin operands: S = min(n, nx + ny - 1) = (3, 2, 1)
    ((MUL, [3], V(0, (2, 2, 1)), V(100, (2, 1, 1)), V(200, (4, 3, 2))),
     "OK nd=1 items=3 inplace=0 ext=[3] xs=[4] ys=[2] ss=[0] rs=[24] rows=1,0,2 slabs=2,1,6 | S=[3,2,1] run=[1,3,2] x=[1,2,2] y=[1,2,1] "
     "xst=[1,2,1] yst=[1,1,0] rst=[1,6,2]"),
    # div by a y with a unit axis: S takes x's length there; a stride-0 divisor against the batch
    ((DIV, [3], V(0, (4, 2, 2)), V(100, (4, 1, 2), bs=[0]), V(200, (4, 3, 2))),
     "OK nd=1 items=3 inplace=0 ext=[3] xs=[16] ys=[0] ss=[0] rs=[24] rows=2,0,2 slabs=4,2,6 | S=[4,2,2] run=[4,2,2] x=[4,2,2] y=[4,1,2] "
     "xst=[4,2,1] yst=[2,0,1] rst=[6,2,1]"),
    # two unit axes: the series row along the slab axis
    ((LOG, [3], V(0, (4, 1, 1)), NOSEED, V(200, (4, 1, 1))),
     "OK nd=1 items=3 inplace=0 ext=[3] xs=[4] ys=[0] ss=[0] rs=[4] rows=0,0,0 slabs=1,0,1 | S=[4,1,1] run=[1,1,4] x=[1,1,4] y=[1,1,1] "
     "xst=[0,1,1] yst=[0,0,0] rst=[0,1,1]"),
    # an empty batch: nothing to do, no stride is looked at
    ((MUL, [3, 0], X, Y, V(200, N, sst=0)), "EMPTY"),
]


def line(case):
    op, batch, x, y, r = case

    def view(v):
        bs = "null" if v["bs"] is None else " ".join(str(s) for s in [len(v["bs"])] + v["bs"])
        return f"{'null' if v['off'] is None else v['off']} {bs} {v['sst']} {v['rst']} {' '.join(str(s) for s in v['shape'])}"

    b = "null 1" if batch is None else " ".join(str(s) for s in [len(batch)] + batch)
    return f"{op} {b} {view(x)} {view(y)} {view(r)} : series3_{('mul', 'div', 'exp', 'log')[op]}"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("series3_args") / "series3_args_main")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "series3_args_main.cpp")]
    for extra in (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []):
        if subprocess.run(base + extra, capture_output=True).returncode != 0:
            continue
        if subprocess.run([exe], input="", capture_output=True, text=True, timeout=60).returncode == 0:  # (it starts here)
            return exe
    pytest.fail("tests/series3_args_main.cpp does not build")


def run_program(exe, cases):
    text = "".join(line(c) + "\n" for c in cases)
    done = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    lines = done.stdout.splitlines()
    assert len(lines) == len(cases), (len(lines), len(cases))
    return lines


def test_rank3_refusals_without_a_device(program):
    for (case, message), got in zip(REFUSED, run_program(program, [c for c, _ in REFUSED])):
        assert got == "E " + message, case


def test_rank3_accepted_calls_collapse_as_recorded(program):
    for (case, plan), got in zip(ACCEPTED, run_program(program, [c for c, _ in ACCEPTED])):
        assert got == plan, case
