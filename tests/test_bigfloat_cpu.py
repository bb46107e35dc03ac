"""`--big-float` without a GPU: the BigFloat number type (src/number/big_float.rs) as the interpreter, the kernels'
element functor and the test oracle restate it, and the interpreter's `--big-float` mode over the oracle backend.

Three restatements are pinned against each other bit for bit: `orcb_scalar_op` (tests/bigfloat_oracle.cpp),
`gfh_bigfloat_op` (genfer_amd/csrc/host/gfh_number.hpp) and EBig (genfer_amd/csrc/gft_elem.hpp, host pass, through
tests/bigfloat_elem_check.hip)."""
import ctypes
import glob
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from genfer_amd import bigfloat
from genfer_amd.reports import NUM, numbers

GENFER = os.path.join(ROOT, "genfer_amd", "csrc", "host", "genfer")
EXAMPLE = os.path.join(GOLDEN, "sgcl", "example.sgcl")
INF, NAN = float("inf"), float("nan")
OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3, "neg": 4, "exp": 5, "log": 6, "normalize": 7, "to_f64": 8, "sqrt": 9,
       "next_up": 10, "next_down": 11, "cmp": 12, "min": 13, "max": 14, "abs": 15, "pow": 16}
ELEM_OPS = ("add", "sub", "mul", "div", "neg", "normalize", "add0")  # bigfloat_elem_check.hip's output order


@pytest.fixture(scope="session")
def orcb_path(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("orcb") / "liborcb.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "bigfloat_oracle.cpp")])
    return so


@pytest.fixture(scope="session")
def orcb(orcb_path):
    L = ctypes.CDLL(orcb_path)
    L.orcb_scalar_op.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


@pytest.fixture(scope="session")
def gfh():
    import genfer_amd

    H = genfer_amd.host_lib()
    H.gfh_bigfloat_op.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return H


@pytest.fixture(scope="session")
def elem_check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("bfcheck") / "bigfloat_elem_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "-o", exe, os.path.join(ROOT, "tests", "bigfloat_elem_check.hip")])
    return exe


def scalar_op(L, fn, op, a, b=None):
    A = np.array(a, dtype=np.float64)
    B = np.array(b if b is not None else (0.0, 0.0), dtype=np.float64)
    out = np.zeros(2)
    assert getattr(L, fn)(OPS[op], A.ctypes.data, B.ctypes.data if b is not None else None, out.ctypes.data) == 0
    return out


def bits(v):
    return tuple(struct.unpack("<q", struct.pack("<d", float(x)))[0] for x in v)


def same(x, y):
    """Bitwise equality of {factor, exponent}; a NaN factor only has to be a NaN on both sides (its sign and payload
    are the hardware's, not the reference's)."""
    if x[0] != x[0] or y[0] != y[0]:
        return x[0] != x[0] and y[0] != y[0] and bits(x[1:]) == bits(y[1:])
    return bits(x) == bits(y)


def run_elem(exe, pairs, tmp_path, device=False):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.asarray(pairs, dtype=np.float64).reshape(-1, 4).tofile(src)
    subprocess.check_call([exe] + (["--device"] if device else []) + [str(src), str(dst)], timeout=300)
    return np.fromfile(dst, dtype=np.float64).reshape(-1, len(ELEM_OPS), 2)


# ---- named vectors -------------------------------------------------------------------------------------------------
# (op, a, b, expected {factor, exponent})
DOC_VECTORS = [  # big_float.rs:14-21 (extract_exponent) through normalize
    ("normalize", (0.0, 0), None, (0.0, 0)),
    ("normalize", (1.0, 0), None, (1.0, 0)),
    ("normalize", (2.0, 0), None, (1.0, 1)),
    ("normalize", (3.0, 0), None, (1.5, 1)),
    ("normalize", (0.5, 0), None, (1.0, -1)),
    ("normalize", (0.75, 0), None, (1.5, -1)),
]
QUIRKS = [
    ("add", (1.0, -1100), (0.0, 0), (0.0, 0)),        # x + 0 drops x when x.exponent <= -1024
    ("add", (0.0, 0), (1.0, -1100), (0.0, 0)),        # ... and 0 + x too
    ("add", (1.0, -1000), (0.0, 0), (1.0, -1000)),
    ("add", (1.5, -1023), (0.0, 0), (1.5, -1023)),    # powi(2, -1023) is a subnormal: rescaled exactly
    ("add", (1.5, -1024), (0.0, 0), (0.0, 0)),
    ("normalize", (-0.0, 0), None, (0.0, 0)),         # normalize(-0) = +0 ...
    ("neg", (0.0, 0), None, (-0.0, 0)),               # ... but neg keeps {-0, 0}
    ("mul", (INF, 5), (1.0, 3), (INF, 8)),            # a non-finite factor keeps its exponent
    ("mul", (1.5, 2000), (1.5, 2000), (1.125, 4001)),
    ("normalize", (2.0 ** -1074, 7), None, (1.0, -1067)),  # subnormal factor
    ("add", (1.0, 5), (1.0, 5), (1.0, 6)),            # exponent tie: self is "bigger"
    ("sub", (1.0, 0), (1.0, 0), (0.0, 0)),
    ("div", (1.0, 0), (0.0, 0), (INF, 0)),
]


@pytest.mark.parametrize("op,a,b,want", DOC_VECTORS + QUIRKS, ids=lambda v: str(v))
def test_named_vectors_three_restatements(op, a, b, want, orcb, gfh, elem_check, tmp_path):
    want = np.array(want, dtype=np.float64)
    for fn, L in (("orcb_scalar_op", orcb), ("gfh_bigfloat_op", gfh)):
        got = scalar_op(L, fn, op, a, b)
        assert same(got, want), (fn, op, a, b, got)
    pair = list(a) + list(b if b is not None else (0.0, 0.0))
    got = run_elem(elem_check, [pair], tmp_path)[0][ELEM_OPS.index(op)]
    assert same(got, want), ("EBig", op, a, b, got)


ULP_BELOW_2 = 1.9999999999999998
# the operations of the moment post-processing (main.rs:256-288 runs in Interval<BigFloat>): (op, a, b, expected)
POST_VECTORS = [
    ("sqrt", (1.0, -1), None, (1.4142135623730951, -1)),   # div_euclid(-1, 2) = -1, rem_euclid = 1: sqrt(2 * 1)
    ("sqrt", (1.0, -3), None, (1.4142135623730951, -2)),
    ("sqrt", (1.0, -2), None, (1.0, -1)),
    ("sqrt", (1.0, 4), None, (1.0, 2)),
    ("sqrt", (1.5, 1), None, (1.7320508075688772, 0)),
    ("next_up", (ULP_BELOW_2, 0), None, (1.0, 1)),          # the factor reaches 2.0: renormalised
    ("next_up", (ULP_BELOW_2, 5), None, (1.0, 6)),
    ("next_down", (1.0, 3), None, (ULP_BELOW_2, 2)),
    ("next_down", (-ULP_BELOW_2, 0), None, (-1.0, 1)),
    ("next_up", (0.0, 0), None, (1.0, -1074)),               # next_up(0) is the least subnormal
    ("abs", (-1.5, 7), None, (1.5, 7)),
    ("pow", (1.5, 3), (2.0, 0), (1.125, 7)),
    ("pow", (1.5, 1000), (3.0, 0), (1.6875, 3001)),
    ("min", (INF, 0), (1.5, 3), (INF, 0)),                   # partial_cmp: exponent 0 < 3, so inf is "less"
    ("max", (-INF, 0), (1.5, -2), (-INF, 0)),
    ("min", (1.0, 2), (1.5, 2), (1.0, 2)),
    ("max", (0.0, 0), (-1.0, 9), (0.0, 0)),                  # a zero operand: the factors decide
]
# partial_cmp (big_float.rs:130-139): -1 less, 0 equal, 1 greater, 2 unordered
CMP_VECTORS = [
    ((1.0, 5), (1.5, 3), 1),
    ((-1.0, 5), (1.0, 3), 1),     # different exponents: the signs are not looked at
    ((0.0, 0), (-1.0, 7), 1),     # a zero on either side: the factors decide
    ((1.0, -3), (0.0, 0), 1),
    ((INF, 0), (1.5, 3), -1),
    ((NAN, 0), (1.0, 0), 2),
    ((1.0, 2), (1.0, 2), 0),
    ((1.25, 2), (1.5, 2), -1),
]


@pytest.mark.parametrize("op,a,b,want", POST_VECTORS, ids=lambda v: str(v))
def test_post_processing_ops(op, a, b, want, orcb, gfh):
    for fn, L in (("orcb_scalar_op", orcb), ("gfh_bigfloat_op", gfh)):
        got = scalar_op(L, fn, op, a, b)
        assert same(got, np.array(want, dtype=np.float64)), (fn, op, a, b, got)


@pytest.mark.parametrize("a,b,want", CMP_VECTORS, ids=lambda v: str(v))
def test_partial_cmp(a, b, want, orcb, gfh):
    for fn, L in (("orcb_scalar_op", orcb), ("gfh_bigfloat_op", gfh)):
        assert scalar_op(L, fn, "cmp", a, b)[0] == want, (fn, a, b)


def test_post_processing_ops_sweep(orcb, gfh):
    """sqrt / next_up / next_down / abs / cmp / min / max of the two host restatements on seeded operands."""
    pairs = random_pairs(20_000, 5)
    for i in range(len(pairs)):
        a, b = pairs[i, :2], pairs[i, 2:]
        for op in ("sqrt", "next_up", "next_down", "abs", "cmp", "min", "max"):
            o, g = scalar_op(orcb, "orcb_scalar_op", op, a, b), scalar_op(gfh, "gfh_bigfloat_op", op, a, b)
            assert same(o, g), (op, a, b, o, g)


def test_ebig_isa(tmp_path):
    """The gfx950 code of EBig (tests/bigfloat_elem_check.hip): frexp / ldexp instructions, no scratch, no calls, no
    pow, and no contracted FMA — the only FMAs are the five of each IEEE f64 division sequence (v_div_fmas_f64)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function",
                           "--save-temps", "-c", "-o", str(tmp_path / "check.o"),
                           os.path.join(ROOT, "tests", "bigfloat_elem_check.hip")], cwd=tmp_path)
    isa = open(glob.glob(str(tmp_path / "*amdgcn-amd-amdhsa*gfx950*.s"))[0]).read()
    code = [l.split()[0] for l in isa.splitlines() if l.startswith("\t") and not l.lstrip().startswith(".")]
    for ins in ("v_frexp_mant_f64", "v_frexp_exp_i32_f64", "v_ldexp_f64"):
        assert any(c.startswith(ins) for c in code), ins
    assert not [c for c in code if c.startswith("scratch_") or c.startswith("buffer_")]
    assert not [c for c in code if c in ("s_swappc_b64", "s_setpc_b64", "s_call_b64")]
    assert ".private_segment_fixed_size: 0" in isa and "pow" not in isa.lower().replace("power", "")
    fmas = sum(c in ("v_fma_f64", "v_fmac_f64_e32", "v_fmac_f64_e64") for c in code)
    assert code.count("v_div_fmas_f64") >= 1 and fmas == 5 * code.count("v_div_fmas_f64"), fmas


def test_to_f64_powi_window(orcb, gfh):
    """to_f64 = factor * powi(2, exponent) with this repository's powi: exactly 2^n down to n = -1023, then 0 (an ldexp
    lowering would keep subnormals down to -1074); +inf from 1024 on; inf * powi(2, -2000) = inf * 0 = NaN."""
    cases = [((1.0, -1023), 2.0 ** -1023), ((1.0, -1024), 0.0), ((1.5, -1030), 0.0), ((1.0, 1023), 2.0 ** 1023),
             ((1.0, 1024), INF), ((1.5, 3), 12.0), ((INF, -2000), NAN), ((-1.0, 0), -1.0)]
    for a, want in cases:
        for fn, L in (("orcb_scalar_op", orcb), ("gfh_bigfloat_op", gfh)):
            got = scalar_op(L, fn, "to_f64", a)[0]
            assert (got != got and want != want) or bits([got]) == bits([want]), (fn, a, got)
            assert (got != got and want != want) or bits([bigfloat.decode(a[0], a[1])]) == bits([want])


def test_exp_log_seeds(orcb, gfh):
    """big_float.rs:147-157, 169-173 (the doc tests), computed by both host restatements identically."""
    e1 = scalar_op(gfh, "gfh_bigfloat_op", "normalize", (np.exp(1.0), 0))
    assert same(scalar_op(gfh, "gfh_bigfloat_op", "exp", (0.0, 0)), (1.0, 0))
    assert same(scalar_op(gfh, "gfh_bigfloat_op", "log", (1.0, 0)), (0.0, 0))
    assert same(scalar_op(gfh, "gfh_bigfloat_op", "log", e1), scalar_op(gfh, "gfh_bigfloat_op", "normalize", (np.log(np.exp(1.0)), 0)))
    for x in (1.0, -1.0, 2.0, -2.0):
        a = scalar_op(gfh, "gfh_bigfloat_op", "normalize", (x, 0))
        for op in ("exp", "log"):
            assert same(scalar_op(gfh, "gfh_bigfloat_op", op, a), scalar_op(orcb, "orcb_scalar_op", op, a)), (op, x)
        # the seed is 2^frac * 2^int, not libm exp: within a few ulps of it
        got = bigfloat.decode(*scalar_op(gfh, "gfh_bigfloat_op", "exp", a))
        assert abs(got - np.exp(x)) <= 4 * np.spacing(np.exp(x))


def random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    f = rng.uniform(1.0, 2.0, size=(n, 2)) * rng.choice([-1.0, 1.0], size=(n, 2))
    e = rng.integers(-3000, 3001, size=(n, 2)).astype(np.float64)
    e[rng.random((n, 2)) < 0.2] = rng.integers(-3, 4, size=1)[0]  # many exponent ties and near-ties
    special = rng.random((n, 2))
    f[special < 0.04] = 0.0
    f[(special >= 0.04) & (special < 0.06)] = -0.0
    f[(special >= 0.06) & (special < 0.08)] = INF
    f[(special >= 0.08) & (special < 0.09)] = -INF
    f[(special >= 0.09) & (special < 0.10)] = NAN
    e[(f == 0.0)] = 0.0
    # one operand a power of two apart from the other: exact cancellations
    k = rng.random(n) < 0.05
    f[k, 1] = -f[k, 0]
    e[k, 1] = e[k, 0]
    return np.stack([f[:, 0], e[:, 0], f[:, 1], e[:, 1]], axis=1)


def test_seeded_sweep_three_restatements(orcb, gfh, elem_check, tmp_path):
    pairs = random_pairs(100_000, 7)
    ebig = run_elem(elem_check, pairs, tmp_path)
    ops = ("add", "sub", "mul", "div", "neg", "normalize")
    bad = []
    for i in range(len(pairs)):
        a, b = pairs[i, :2], pairs[i, 2:]
        for op in ops:
            o = scalar_op(orcb, "orcb_scalar_op", op, a, b)
            g = scalar_op(gfh, "gfh_bigfloat_op", op, a, b)
            k = ebig[i][ELEM_OPS.index(op)]
            if not (same(o, g) and same(o, k)):
                bad.append((op, tuple(a), tuple(b), tuple(o), tuple(g), tuple(k)))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:3]}"


def test_encode_decode_roundtrip():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(1000) * 10.0 ** rng.integers(-300, 300, 1000),
                        [0.0, -0.0, INF, -INF, 2.0 ** -1074, 2.0 ** -1022, 1.7976931348623157e308]])
    f, e = bigfloat.encode(x)
    fin = np.isfinite(x) & (x != 0)
    assert np.all((np.abs(f[fin]) >= 1.0) & (np.abs(f[fin]) < 2.0))
    assert np.all(e[x == 0] == 0) and np.all(f[x == 0] == 0) and not np.any(np.signbit(f[x == 0]))
    # decode is to_f64: exact inside the powi window, so every normal f64 comes back
    normal = fin & (np.abs(x) >= 2.0 ** -1022)
    assert np.array_equal(bigfloat.decode(f, e)[normal], x[normal])


# ---- the interpreter -----------------------------------------------------------------------------------------------
def genfer(args, backend, timeout=300):
    env = dict(os.environ, GENFER_BACKEND=backend)
    return subprocess.run([GENFER] + args, capture_output=True, text=True, env=env, timeout=timeout)


def test_cli_accepts_big_float(orcb_path):
    r = genfer(["--big-float", "--no-timing", EXAMPLE], orcb_path + ":orc")
    assert r.returncode == 0, r.stderr + r.stdout
    assert "Expected value:            E = 8.999999999999998\n" in r.stdout


def test_cli_big_float_refused_without_bigfloat_family():
    """libgftaylor has no gftb_ family: --big-float on the default backend is refused by name, before any run."""
    env = {k: v for k, v in os.environ.items() if k != "GENFER_BACKEND"}
    r = subprocess.run([GENFER, "--big-float", "--no-timing", EXAMPLE], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode != 0
    assert "flag --big-float is out of scope for this backend" in r.stderr + r.stdout
    assert "no BigFloat TaylorPoly family (gftb_*)" in r.stderr + r.stdout


def test_cli_big_float_bounds_refused(orcb_path):
    r = genfer(["--big-float", "--bounds", "--no-timing", EXAMPLE], orcb_path + ":orc")
    assert r.returncode != 0
    assert "--big-float together with --bounds" in r.stdout + r.stderr


def test_cli_other_number_modes_still_refused(orcb_path):
    for flag in ("--rational", "-s"):
        r = genfer([flag, "--no-timing", EXAMPLE], orcb_path + ":orc")
        assert r.returncode != 0 and "out of scope" in r.stdout + r.stderr


def test_interval_bigfloat_division_quirk_pinned(orcb_path):
    """Interval<T>::div (interval.rs:199-234) seeds its bounds with T::infinity() = {inf, 0}, and BigFloat's
    partial_cmp (big_float.rs:130-139) orders different exponents by exponent alone, infinities included.  So a
    quotient with exponent > 0 never replaces the lower seed and one with exponent < 0 never replaces the upper one;
    the standardised moments and the normalised masses of a --big-float report are centres of such intervals.  The
    interpreter reproduces that; this pins it so a change is deliberate."""
    r = genfer(["--big-float", "--no-timing", EXAMPLE], orcb_path + ":orc")
    assert "Skewness (3rd std moment): S = -8.988465674311579e307\n" in r.stdout
    assert "Kurtosis (4th std moment): K = 8.988465674311579e307\n" in r.stdout


# Report lines computed through Interval<BigFloat> division (the quirk above): not comparable with the f64 report.
DIVIDED = ("Skewness", "Kurtosis", "Normalized:", "p(n) / Z")

SNAPSHOTS = sorted(f for f in glob.glob(os.path.join(GOLDEN, "sgcl", "**", "*.sgcl"), recursive=True)
                   if os.path.exists(f[:-5] + ".expect") and os.sep + "slow" + os.sep not in f)


def flags_of(path):
    first = open(path).readline()
    return first[len("# flags:"):].strip() if first.startswith("# flags:") else ""


def without_divided(text):
    return "\n".join(l for l in text.splitlines() if not any(k in l for k in DIVIDED)) + "\n"


# Both switchpoint programs print unnormalised masses far below their terms: BigFloat and f64 disagree there in the
# third digit (p(11): 1.8204e-89 vs 1.8224e-89), and from p(82) on BigFloat prints 0.0 where f64 prints 2.3e-87.  Their
# moments are compared as everywhere else; their masses are not.
DIVERGENT = {os.path.join("test_expect", "real_world", "cont_switchpoint.sgcl"),
             os.path.join("neurips2023", "approx", "switchpoint", "switchpoint.sgcl")}


@pytest.mark.parametrize("path", [p for p in SNAPSHOTS if not {"-b", "--bounds"} & set(flags_of(p).split())],
                         ids=lambda p: os.path.relpath(p, os.path.join(GOLDEN, "sgcl")))
def test_snapshots_big_float_on_oracle(path, orcb_path):
    import genfer_amd

    rc, text, _ = genfer_amd.run_sgcl_with_backend(open(path).read(), "--no-timing --big-float " + flags_of(path), orcb_path, "orcb_")
    assert rc == 0, text
    got, want = without_divided(text).splitlines(), without_divided(open(path[:-5] + ".expect").read()).splitlines()
    assert len(got) == len(want)
    divergent = os.path.relpath(path, os.path.join(GOLDEN, "sgcl")) in DIVERGENT
    for g, w in zip(got, want):
        assert NUM.sub("#", g) == NUM.sub("#", w), (g, w)
        # primary quantities only: BigFloat rounds differently from f64 (exp / log seeds, rescaled sums), and the
        # central moments are differences of raw moments that amplify those last-bit differences
        primary = ("Total measure", "Expected value", "raw moment") + (() if divergent else ("p(",))
        if any(k in w for k in primary) and "<=" not in w:
            for a, b in zip(numbers(g), numbers(w)):
                assert (a != a and b != b) or a == b or abs(a - b) <= 1e-8 * abs(b), (g, w)
