"""gft_pair_plan.hpp (the row-pair product's slab ranges, lanes and phase-1 grids) against its recorded table and, by brute
force, against the index arithmetic of k_pair_sums — on the CPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_plan_table_and_grids():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pair_plan_check")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genfer_amd", "csrc"),
                               os.path.join(ROOT, "tests", "pair_plan_check.cpp"), "-o", exe])
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "pair_plan_table.txt")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.rstrip().endswith("pair_plan ok")
