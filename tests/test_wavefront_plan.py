"""gft_wavefront_plan.hpp (which persistent wavefront runs a div / log / exp recurrence, and how) against its table, on the CPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wavefront_plan_table():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "wavefront_plan_check")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genfer_amd", "csrc"),
                               os.path.join(ROOT, "tests", "wavefront_plan_check.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "wavefront_plan ok" in r.stdout
