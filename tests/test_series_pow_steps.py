"""pow's step planner (series_pow_steps, genfer_amd/csrc/gft_series_args.hpp) without a device: tests/series_pow_steps_main.cpp, a
stand-alone program built with the host compiler -- under AddressSanitizer and UndefinedBehaviorSanitizer where the compiler has
them and the program runs with them.  The steps it prints are compared, one by one, with the reference's square-and-multiply
loop (multivariate_taylor.rs:441-450) replayed here on powers of x and their stored shapes."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

EXPONENTS = [0, 1, 2, 3, 5, 6, 7, 8, 13, 31, 64, 2 ** 31, 2 ** 32 - 1]
SHAPES = [  # the stored shape of x -> the orders n
    ((1, 1, 3), (1, 1, 8)),
    ((1, 2, 3), (1, 3, 8)),
    ((2, 1, 3), (3, 2, 5)),
    ((1, 1, 1), (2, 2, 2)),
    ((2, 3, 4), (2, 3, 4)),  # already n: nothing grows
]
CASES = [(e, nx, n) for nx, n in SHAPES for e in EXPONENTS]


def reference_products(e, nx, n):
    """The products of the loop  res = 1; base = x; while e > 0: if e & 1: res *= base; base *= base; e >>= 1  in order, each as
    (left, right, writes) with an operand as (power of x, stored shape) and `writes` as (power, compact shape): the product of
    stored shapes a and b is stored at min(a + b - 1, n) per axis (sum_shape).  The square after the last multiplication is never
    read and is not a product."""
    def compact(a, b):
        return tuple(min(p + q - 1, m) for p, q, m in zip(a, b, n))

    res, base = (0, (1, 1, 1)), (1, tuple(nx))
    out = []
    while e > 0:
        if e & 1:
            new = (res[0] + base[0], compact(res[1], base[1]))
            out.append((res, base, new))
            res = new
        e >>= 1
        if e > 0:
            new = (2 * base[0], compact(base[1], base[1]))
            out.append((base, base, new))
            base = new
    return out, res


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("series_pow_steps") / "series_pow_steps_main")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "series_pow_steps_main.cpp")]
    for extra in (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []):
        if subprocess.run(base + extra, capture_output=True).returncode != 0:
            continue
        if subprocess.run([exe], input="", capture_output=True, text=True, timeout=60).returncode == 0:  # (it starts here)
            return exe
    pytest.fail("tests/series_pow_steps_main.cpp does not build")


@pytest.fixture(scope="module")
def planned(program):
    """{case: its steps as (a, b, out, sa, sb, L, last)}, from one run of the program"""
    text = "".join(f"{e} {' '.join(map(str, nx))} {' '.join(map(str, n))}\n" for e, nx, n in CASES)
    done = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    lines = iter(done.stdout.splitlines())
    out = {}
    for case in CASES:
        head = next(lines).split()
        assert head[0] == "steps", head
        steps = []
        for _ in range(int(head[1])):
            t = next(lines).split()
            v = [int(s) for s in t[3:]]
            steps.append((t[0], t[1], t[2], tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:9]), bool(v[9])))
        out[case] = steps
    assert next(lines, None) is None
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"e{c[0]}-{'x'.join(map(str, c[1]))}-n{'x'.join(map(str, c[2]))}")
def test_steps_are_the_reference_loop(planned, case):
    e, nx, n = case
    steps = planned[case]
    want, final = reference_products(e, nx, n)
    assert len(steps) == (bin(e).count("1") + e.bit_length() - 1 if e else 0)  # popcount(e) + floor(log2 e)
    assert len(steps) == len(want)
    holds = {"unit": 0, "ws0": 1}  # slot -> the power of x it holds: [1.0] and the copy of x
    shape = {0: (1, 1, 1), 1: tuple(nx)}
    res_p, base_p = 0, 1  # what the loop still reads
    for i, ((a, b, out, sa, sb, L, last), (left, right, new)) in enumerate(zip(steps, want)):
        # the operand roles in the reference's order: accumulator times base, or base times base
        assert (holds[a], holds[b]) == (left[0], right[0]), (i, a, b)
        assert (sa, sb) == (left[1], right[1]) == (shape[holds[a]], shape[holds[b]]), i
        assert L == new[1], i
        assert out not in (a, b) and out != "unit", i
        assert last == (i == len(steps) - 1) and (out == "result") == last, i
        if left is not right:
            res_p = new[0]
        else:
            base_p = new[0]
        holds[out] = new[0]
        shape[new[0]] = new[1]
        # the output displaced nothing the loop still reads (the last product ends the loop: base is dead by then)
        live = {res_p} if last else {res_p, base_p}
        assert live <= set(holds.values()), (i, holds, live)
        assert set(holds) <= {"unit", "ws0", "ws1", "ws2", "result"}
    if e:
        assert holds["result"] == e == final[0] and steps[-1][5] == final[1]
        assert [s[2] for s in steps].count("result") == 1
