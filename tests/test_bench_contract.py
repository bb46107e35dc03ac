"""bench.py's static contract, checked without a GPU: the programs its `e2e` rows time exist as committed fixtures, the
clock sampler is a child that is started before anything can have initialised the GPU, and the JSON keys the driver
reads are spelled in the source."""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_source():
    with open(os.path.join(ROOT, "bench.py")) as f:
        return f.read()


def test_e2e_programs_are_committed_fixtures():
    tree = ast.parse(_bench_source())
    progs = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "E2E_PROGRAMS" for t in node.targets):
            progs = ast.literal_eval(node.value)
    assert progs, "E2E_PROGRAMS not found"
    names = set()
    for name, rel, flags, cpu_runs, stored, recorded in progs:
        assert name not in names
        names.add(name)
        assert os.path.isfile(os.path.join(ROOT, "tests", "golden", "sgcl", rel)), rel
        assert isinstance(flags, str) and isinstance(cpu_runs, int) and cpu_runs >= 0
        # every row has a checker at the size it is timed at: an oracle run in the same call, or a committed oracle report
        assert cpu_runs > 0 or stored, name
        if stored:
            assert os.path.isfile(os.path.join(ROOT, "tests", "golden", "c3_limit100", stored)), stored
        if cpu_runs == 0:  # no CPU seconds measured in the run: the recorded figure names its source
            assert recorded and recorded[0] > 0 and "profiles/" in recorded[1]
    assert {"hmm", "mixture", "three_populations", "four_populations", "hmm_bounds", "mixture_bounds"} <= names


def test_clock_helper_starts_before_the_gpu_is_touched():
    src = _bench_source()
    main = src[src.index("def main():"):]
    assert main.index("start_clock_helper()") < main.index("import torch"), "the rocm-smi helper must be forked before HIP can be initialised"
    assert "subprocess.Popen" not in src[src.index("def sclk_under_load"):src.index("def main():")], "no fork + exec after GPU initialisation"


def test_nothing_spawns_a_process_after_gpu_initialisation():
    """A process that has initialised HIP must not fork + exec on this pool: the oracle library is built (if missing)
    by ensure_oracle() BEFORE `import torch`; cpu_baseline / e2e_seconds / main's body after that point spawn nothing."""
    src = _bench_source()
    main = src[src.index("def main():"):]
    assert main.index("ensure_oracle()") < main.index("import torch")
    for fn in ("def cpu_baseline(", "def cpu_baseline_all_cores(", "def e2e_seconds("):
        body = src[src.index(fn):]
        body = body[:body.index("\n\n\n")]
        assert "subprocess" not in body and "os.system" not in body and "Popen" not in body, fn
    after = main[main.index("import torch"):]
    assert "subprocess" not in after and "os.system" not in after and "Popen(" not in after


def test_smoke_builds_the_oracle_before_it_initialises_the_gpu():
    """__graft_entry__.smoke(): _oracle_cls() may spawn `make`; it must run before genfer_amd.init() (the same rule)."""
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        src = f.read()
    smoke = src[src.index("def smoke()"):]
    smoke = smoke[:smoke.index("\n\n\n")]
    assert smoke.index("_oracle_cls()") < smoke.index("genfer_amd.init("), "build the oracle before the GPU is initialised"
    after = smoke[smoke.index("genfer_amd.init("):]
    assert "subprocess" not in after and "os.system" not in after and "_oracle_cls" not in after


def test_plain_run_does_only_the_headline():
    """Everything beside the timed steps that costs time of its own (oracle build, clock sampler, CPU baselines and parity,
    e2e seconds, the N > 1 self-test and single-GPU comparison) sits under a branch on `args.full` in main()."""
    tree = ast.parse(_bench_source())
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    extras = {"ensure_oracle", "start_clock_helper", "sclk_under_load", "cpu_baseline", "cpu_baseline_all_cores", "e2e_seconds",
              "gft_dist_selftest", "gpu_conv_slabs"}
    found = set()

    def mentions_full(expr):
        return any(isinstance(n, ast.Attribute) and n.attr == "full" for n in ast.walk(expr))

    def visit(node, guarded):
        if isinstance(node, ast.Call):
            f = node.func
            name = f.attr if isinstance(f, ast.Attribute) else getattr(f, "id", None)
            if name in extras:
                assert guarded, f"{name}() runs without --full (line {node.lineno})"
                found.add(name)
        if isinstance(node, ast.If) and mentions_full(node.test):
            visit(node.test, guarded)
            for child in node.body + node.orelse:
                visit(child, True)
            return
        for child in ast.iter_child_nodes(node):
            visit(child, guarded)

    visit(main, False)
    assert found == extras, extras - found


def test_e2e_rows_carry_a_parity_verdict():
    src = _bench_source()
    body = src[src.index("def e2e_seconds("):src.index("_CLOCK_HELPER")]
    assert "first_difference" in body and '"parity"' in body and "failed = True" in body


def test_contract_keys_are_present():
    src = _bench_source()
    for key in ('"metric"', '"value"', '"unit"', '"n_gpus"', '"steps"', '"warmup"', '"ms_per_step"', '"higher_is_better"', '"scaling"',
                '"vs_baseline"', '"dtype"', '"data"', '"config"', '"roofline"', '"cpu_baseline"', '"bound"', '"achieved"', '"peak"', '"frac"', '"traffic"'):
        assert key in src, key


def _bench_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_the_arrays_within_budget(tmp_path, monkeypatch):
    import numpy as np

    bench = _bench_module()
    small = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    rec = bench.dump_outputs(str(tmp_path / "a"), {"z": small})
    assert np.array_equal(np.load(tmp_path / "a" / "z.npy"), small) and "sample" not in rec["arrays"]["z"]

    # an array above its share of the budget becomes a fixed sample: the same values in every run, within the budget
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 * 1024)
    big = np.random.default_rng(7).random((64, 64, 8))
    for d in ("b", "c"):
        rec = bench.dump_outputs(str(tmp_path / d), {"z": big, "w": big.astype(np.float32)})
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= bench.DUMP_BUDGET_BYTES
    for name, dtype in (("z", np.float64), ("w", np.float32)):
        got = np.load(tmp_path / "b" / f"{name}.npy")
        assert got.dtype == dtype and got.ndim == 1 and 0 < got.size < big.size and "sample" in rec["arrays"][name]
        assert np.array_equal(got, np.load(tmp_path / "c" / f"{name}.npy"))
        k = got.size
        idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(big.size, k, replace=False))
        assert np.array_equal(got, big.astype(dtype).reshape(-1)[idx])


def test_dump_outputs_takes_the_last_timed_step():
    """The snapshot is taken after the timed loop and before the untimed steps (clock sample, CPU parity) run the product again."""
    src = _bench_source()
    main = src[src.index("def main():"):]
    timed = main.index("for _ in range(args.steps):")
    snap = main.index("last_z = z.cpu()")
    assert timed < snap < main.index("sclk_under_load(") and snap < main.index("cpu_baseline(shape")
