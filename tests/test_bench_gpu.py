"""bench.py on the GPU at the debug size: a plain run prints the headline line and nothing that needs runs of its own;
--full adds the CPU baselines and the oracle parity sample.  Both dump the same product."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, name, *flags):
    out_dir = str(tmp_path / name)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "small",
           "--dump-outputs", out_dir, *flags]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "GMAC/s" and d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 2 and d["warmup"] == 1
    assert d["roofline"]["kernel_ms"] > 0
    return d, np.load(os.path.join(out_dir, "z.npy"))


@pytest.mark.gpu
def test_plain_and_full_runs(tmp_path):
    plain, z_plain = _bench(tmp_path, "plain")
    assert plain["full"] is False and plain["cpu_baseline"] is None
    for key in ("cpu_baseline_all_cores", "parity_max_rel_err_vs_oracle_sample", "e2e"):
        assert key not in plain, key
    assert plain["roofline"]["during_timed_loop"] is None and "sclk_mhz_under_load" not in plain["roofline"]

    full, z_full = _bench(tmp_path, "full", "--full", "--no-clock")
    assert full["full"] is True
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline_all_cores"]["value"] > 0
    assert full["parity_max_rel_err_vs_oracle_sample"] <= 1e-10

    assert z_plain.shape == z_full.shape == (32, 32, 32)
    assert np.all(np.abs(z_plain - z_full) <= 1e-10 * np.abs(z_full))
