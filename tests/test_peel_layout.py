"""gft_peel_layout.hpp (the workspace of a peeled tiled product: ticket counters, the three launches' own partial slabs,
packed operands, gathered leftover operands): disjoint, aligned, inside `need`, monotone in every slot count — on the
CPU, in a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_peel_layout_regions():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "peel_layout_check")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I",
                               os.path.join(ROOT, "genfer_amd", "csrc"), os.path.join(ROOT, "tests", "peel_layout_check.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.rstrip().endswith("peel_layout ok")
