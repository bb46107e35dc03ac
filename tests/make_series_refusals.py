"""Writes tests/series_refusals.json: every refusal of the batched series layer as (case, exception type, whole message).

The table pins the messages across refactors of the two host layers, so it is recorded from a commit whose behaviour is the
standard (the parent of the commit that changes the layers) and replayed by tests/test_series_refusals.py:

    python tests/make_series_refusals.py --python     # the Python layer: no device needed
    python tests/make_series_refusals.py --c          # the C layer: raw calls of the entry points, on the GPU
    python tests/make_series_refusals.py --accepted tests/series_args_main   # accepted calls: the collapsed batch, from the
                                                      # compiled tests/series_args_main.cpp (reviewed by eye, then pinned)

Each mode rewrites its own part of the file and keeps the others.  Cases are data: the functions below turn one into the call.

The C layer's cases are one call each in the descriptor's terms (genfer_amd/csrc/gft_series_args.hpp): an op, the element width
w, the rank, e / var / k, the batch, and three views (x, then y or the seeds, then the result) of one device buffer of BUFFER
doubles -- `off` doubles into it (None: a null pointer), the stride array `bs` (None: contiguous), the row stride and the two
lengths.  No case launches a kernel: every one is refused, or is an empty batch (message None: the call returns 0).
"""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "series_refusals.json")
BUFFER = 8192 + 256  # the result of the 13-axis case alone is 2^13 doubles; everything else lives in a few hundred

OPS = ["mul", "div", "exp", "log", "compose", "pow", "corr", "compose_adj", "derivative", "taylor_expansion_of_coeff", "shift_down",
       "evaluate_all_one"]
BINARY, SEEDED, OBSERVE = ("mul", "div", "compose", "corr", "compose_adj"), ("exp", "log"), OPS[8:]


def V(off, len1, len0=1, bs=None, rst=0):
    return {"off": off, "bs": None if bs is None else list(bs), "rst": rst, "len0": len0, "len1": len1}


def call(op, x, y, r, batch=(), w=1, rank2=False, e=0, var=0, k=0, nbatch=None, device_only=False):
    """nbatch: only where it differs from len(batch) (batch None: a null batch pointer).  device_only: the refusal is the
    pointer check's, which the stand-alone program does not have."""
    c = {"op": op, "w": w, "rank2": rank2, "e": e, "var": var, "k": k, "batch": None if batch is None else list(batch), "x": x, "y": y, "r": r}
    if nbatch is not None:
        c["nbatch"] = nbatch
    if device_only:
        c["device_only"] = True
    return c


NOSEED = V(None, 1)


def c_cases():
    out = []

    def add(*a, **k):
        out.append(call(*a, **k))

    x8, y8, r8 = V(0, 8), V(16, 8), V(32, 8)
    # ---- the shape rules, rank 1, the result is the long side
    add("mul", x8, y8, V(32, 0))
    add("mul", x8, y8, V(32, 4097))
    add("mul", x8, y8, V(32, 2049), w=2)
    add("exp", x8, NOSEED, V(32, 4097))
    add("mul", V(0, 0), y8, r8)
    add("mul", x8, V(16, 0), r8)
    add("log", V(0, 0), NOSEED, r8)
    add("pow", V(0, 0), V(None, 1), r8, e=3)
    add("mul", V(0, 9), y8, r8)
    add("div", x8, V(16, 9), r8)
    add("compose", x8, V(16, 9), r8, w=2)
    add("pow", V(0, 9), V(None, 1), r8, e=2)
    # ---- rank 1, transposed: x is the long side
    add("corr", x8, y8, V(32, 0))
    add("compose_adj", x8, y8, V(32, 0))
    add("corr", V(0, 4097), y8, r8)
    add("compose_adj", V(0, 4097), y8, r8)
    add("corr", x8, V(16, 0), r8)
    add("corr", V(0, 0), y8, V(32, 1))
    add("corr", x8, y8, V(32, 9))
    add("compose_adj", x8, y8, V(32, 9))
    add("corr", x8, V(16, 9), r8)
    add("compose_adj", x8, V(16, 9), r8)
    # ---- rank 2, the result is the long side
    x2, y2, r2 = V(0, 8, 3, rst=8), V(32, 8, 3, rst=8), V(64, 8, 3, rst=8)  # 3 x 8 coefficients per item
    add("mul", x2, y2, dict(r2, len0=0), rank2=True)
    add("mul", x2, y2, dict(r2, len1=0), rank2=True)
    add("mul", x2, y2, dict(r2, len0=17, len1=241), rank2=True)
    add("mul", x2, y2, dict(r2, len0=2, len1=1025), rank2=True, w=2)
    add("div", x2, y2, dict(r2, len0=4097, len1=1), rank2=True)
    add("exp", x2, NOSEED, dict(r2, len0=1, len1=4097), rank2=True)
    add("mul", dict(x2, len0=0), y2, r2, rank2=True)
    add("mul", x2, dict(y2, len1=0), r2, rank2=True)
    add("exp", dict(x2, len1=0), NOSEED, r2, rank2=True, w=2)
    add("mul", dict(x2, len0=4), y2, r2, rank2=True)
    add("mul", dict(x2, len1=9), y2, r2, rank2=True)
    add("div", x2, dict(y2, len0=4), r2, rank2=True, w=2)
    add("compose", x2, dict(y2, len1=9), r2, rank2=True)
    add("pow", dict(x2, len1=9), V(None, 1), r2, rank2=True, e=2)
    # ---- rank 2, transposed
    add("corr", x2, y2, dict(r2, len0=0), rank2=True)
    add("compose_adj", x2, y2, dict(r2, len1=0), rank2=True)
    add("corr", dict(x2, len0=17, len1=241), y2, r2, rank2=True)
    add("compose_adj", dict(x2, len0=4097, len1=1), y2, r2, rank2=True, var=1)
    add("corr", x2, dict(y2, len0=0), r2, rank2=True)
    add("corr", dict(x2, len1=0), y2, r2, rank2=True)
    add("corr", x2, y2, dict(r2, len0=4), rank2=True)
    add("compose_adj", x2, y2, dict(r2, len1=9), rank2=True)
    add("corr", x2, dict(y2, len1=9), r2, rank2=True)
    add("compose_adj", x2, dict(y2, len0=4), r2, rank2=True, var=1)
    # ---- var
    add("compose", x2, y2, r2, rank2=True, var=2)
    add("compose", x2, y2, r2, rank2=True, var=-1, w=2)
    add("compose_adj", x2, y2, r2, rank2=True, var=2)
    # ---- the observation ops: x is the long side, the result's shape follows from k
    for op in ("derivative", "taylor_expansion_of_coeff", "shift_down"):
        add(op, V(0, 0), NOSEED, V(32, 8), k=1)
        add(op, x8, NOSEED, V(32, 7), k=8)
        add(op, x8, NOSEED, V(32, 8), k=1)
    add("derivative", V(0, 4097), NOSEED, V(32, 4096), k=1)
    add("shift_down", V(0, 2049), NOSEED, V(32, 2048), k=1, w=2)
    add("evaluate_all_one", V(0, 0), NOSEED, V(32, 1))
    add("evaluate_all_one", V(0, 4097), NOSEED, V(32, 1))
    add("evaluate_all_one", V(0, 2049), NOSEED, V(32, 1), w=2)
    add("derivative", dict(x2, len0=0), NOSEED, r2, rank2=True, k=1)
    add("derivative", dict(x2, len0=17, len1=241), NOSEED, r2, rank2=True, k=1)
    add("taylor_expansion_of_coeff", dict(x2, len0=2, len1=1025), NOSEED, r2, rank2=True, k=1, w=2)
    add("evaluate_all_one", dict(x2, len0=17, len1=241), NOSEED, V(64, 1), rank2=True)
    add("evaluate_all_one", dict(x2, len1=0), NOSEED, V(64, 1), rank2=True)
    add("shift_down", x2, NOSEED, r2, rank2=True, var=2, k=1)
    add("derivative", x2, NOSEED, r2, rank2=True, var=-1, k=1, w=2)
    add("derivative", x2, NOSEED, dict(r2, len0=2), rank2=True, var=0, k=3)
    add("derivative", x2, NOSEED, dict(r2, len1=7), rank2=True, var=1, k=8)
    add("shift_down", x2, NOSEED, r2, rank2=True, var=0, k=1)
    add("shift_down", x2, NOSEED, dict(r2, len0=2, len1=7), rank2=True, var=1, k=1)
    add("taylor_expansion_of_coeff", x2, NOSEED, dict(r2, len0=2, len1=7), rank2=True, var=0, k=1, w=2)
    # ---- the batch
    add("mul", x8, y8, r8, batch=[1] * 33)
    add("mul", x8, y8, r8, batch=None, nbatch=1)
    add("mul", x8, y8, r8, batch=[65536, 32768])
    add("derivative", x8, NOSEED, V(32, 7), k=1, batch=[32768, 65536], w=2)
    add("mul", dict(x8, bs=[-8, 8]), y8, dict(r8, bs=[0, 0]), batch=[3, 0])  # an empty batch: returns 0 before any stride is looked at
    # ---- negative strides: the row axis, the plane axis, a batch axis, on every operand
    b = [3]
    add("mul", dict(x8, bs=[-8]), y8, r8, batch=b)
    add("mul", x8, dict(y8, bs=[-8]), r8, batch=b)
    add("mul", x8, y8, dict(r8, bs=[-8]), batch=b)
    add("exp", x8, V(100, 1, bs=[-1]), r8, batch=b)
    add("compose", dict(x8, bs=[8, -1]), y8, r8, batch=[3, 2])
    add("corr", x8, dict(y8, bs=[-8]), r8, batch=b)
    add("compose_adj", dict(x8, bs=[-8]), y8, r8, batch=b)
    add("mul", dict(x8, bs=[-24, 8]), y8, r8, batch=b, w=2)
    add("mul", x8, y8, dict(r8, bs=[-24, 8]), batch=b, w=2)
    add("log", x8, V(100, 1, bs=[-3, 1]), r8, batch=b, w=2)
    add("mul", dict(x2, rst=-8), y2, r2, rank2=True)
    add("mul", x2, dict(y2, rst=-8), r2, rank2=True)
    add("mul", x2, y2, dict(r2, rst=-8), rank2=True, w=2)
    add("derivative", dict(x2, rst=-8), NOSEED, dict(r2, len0=2), rank2=True, k=1)
    # ---- the result's elements are distinct addresses
    add("mul", x8, y8, dict(r8, bs=[0, 8]), batch=b, w=2)
    add("mul", x8, y8, dict(r8, bs=[0]), batch=b)
    add("mul", x8, y8, dict(r8, bs=[8, 0]), batch=[1, 3])
    add("mul", x2, y2, dict(r2, rst=0), rank2=True)
    add("evaluate_all_one", x8, NOSEED, V(32, 1, bs=[0]), batch=b)
    add("mul", x8, y8, dict(r8, bs=[4]), batch=b)  # rows 4 apart, 8 long
    add("mul", x2, y2, dict(r2, rst=4), rank2=True)  # the rows of an item overlap each other
    add("mul", x2, y2, dict(r2, bs=[16]), rank2=True, batch=b)  # items 16 apart, 24 long
    add("mul", x8, y8, dict(r8, bs=[4, 8]), batch=b, w=2)  # the hi plane starts inside the lo plane
    add("mul", x8, y8, dict(r8, bs=[3, 8]), batch=[3, 2])  # two batch axes interleave
    # ---- the pointer check (needs the device)
    add("mul", V(None, 8), y8, r8, device_only=True)
    add("mul", x8, V(None, 8), r8, device_only=True)
    add("mul", x8, y8, V(None, 8), device_only=True)
    add("corr", x8, V(None, 8), r8, device_only=True)
    add("derivative", V(None, 8), NOSEED, V(32, 7), k=1, device_only=True, w=2)
    # ---- overlap: the result may alias an operand only as the same view
    add("mul", x8, y8, V(4, 8))
    add("mul", x8, y8, V(20, 8))
    add("exp", x8, V(35, 1), r8)
    add("log", x8, V(32, 1), r8, w=2)
    add("pow", x8, V(None, 1), V(4, 8), e=2)
    add("compose", dict(x8, bs=[8]), dict(y8, off=64, bs=[8]), V(0, 8, bs=[16]), batch=[2])  # the same start, another view
    add("corr", x8, y8, V(16, 8))  # the transposed ops' second operand, as the same view
    add("compose_adj", x8, y8, V(16, 8))
    add("corr", x2, y2, y2, rank2=True)
    add("compose_adj", x2, y2, y2, rank2=True, var=1)
    add("corr", x8, y8, V(4, 4))
    add("mul", x2, y2, dict(r2, off=8), rank2=True)
    add("mul", x2, y2, dict(r2, off=40), rank2=True, w=2)
    add("derivative", x8, NOSEED, V(1, 7), k=1)
    add("evaluate_all_one", x2, NOSEED, V(23, 1), rank2=True)
    # ---- more non-contiguous batch axes than the kernels take: x alternates stride 1 and 0, so no two axes merge
    alt = [i % 2 for i in range(13)]
    add("mul", V(8200, 1, bs=alt), V(8210, 1, bs=alt), V(0, 1), batch=[2] * 13)
    add("mul", V(8200, 1, bs=[4] + alt[:12]), V(8210, 1, bs=[4] + alt[:12]), V(0, 1), batch=[2] * 12, w=2)
    add("pow", V(8200, 1, bs=alt[:12]), V(None, 1), V(0, 1), batch=[2] * 12, rank2=True, e=2)
    add("pow", V(8200, 1, bs=[4] + alt[:11]), V(None, 1), V(0, 1), batch=[2] * 11, rank2=True, e=2, w=2)
    add("evaluate_all_one", V(8200, 2, bs=alt), NOSEED, V(0, 1), batch=[2] * 13)
    return out


def accepted_cases():
    x8, y8, r8 = V(0, 8), V(100, 8), V(200, 8)
    return [
        call("mul", x8, y8, r8, batch=[3, 4]),  # contiguous: one merged axis
        call("mul", x8, dict(y8, bs=[0, 0]), r8, batch=[3, 4]),  # y is one series against the batch
        call("mul", dict(x8, bs=[64, 8]), dict(y8, bs=[0, 8]), r8, batch=[3, 4]),  # two axes that do not merge
        call("mul", x8, y8, x8, batch=[3, 4]),  # in place: the result is x, the same view
        call("div", V(0, 8, bs=[0, 32, 8]), V(100, 8), V(400, 8), batch=[3, 4], w=2),  # x is a point interval: plane stride 0
        call("exp", x8, V(300, 1), r8, batch=[3, 4]),  # seeds
        call("mul", V(0, 8, 3, rst=8), V(100, 8, 3, rst=8), V(200, 8, 3, bs=[48], rst=16), batch=[2], rank2=True),  # rank 2, the result's rows apart
        call("mul", x8, y8, r8, batch=[3, 0]),  # an empty batch
    ]


# ---- a case as a line of tests/series_args_main.cpp and as a raw call of the entry point ------------------------------------


def fn_name(c):
    return ("interval " if c["w"] == 2 else "") + ("series2_" if c["rank2"] else "series_") + c["op"]


def entry_name(c):
    return ("gfti_" if c["w"] == 2 else "gft_") + ("series2_" if c["rank2"] else "series_") + c["op"]


def _nbatch(c):
    return c.get("nbatch", 0 if c["batch"] is None else len(c["batch"]))


def _var(c):  # what the entry points put into the descriptor: at rank 1 the observation ops act on axis 1, the series axis
    return c["var"] if c["rank2"] else (1 if c["op"] in OBSERVE else 0)


def program_line(c):
    def view(v):
        bs = "null" if v["bs"] is None else " ".join(str(s) for s in [len(v["bs"])] + v["bs"])
        return f"{'null' if v['off'] is None else v['off']} {bs} {v['rst']} {v['len0']} {v['len1']}"

    batch = f"null {_nbatch(c)}" if c["batch"] is None else " ".join(str(s) for s in [len(c["batch"])] + c["batch"])
    return (f"{OPS.index(c['op'])} {c['w']} {int(c['rank2'])} {c['e']} {_var(c)} {c['k']} {batch} "
            f"{view(c['x'])} {view(c['y'])} {view(c['r'])} : {fn_name(c)}")


def run_program(exe, cases):
    """the lines the stand-alone program prints for the cases"""
    text = "".join(program_line(c) + "\n" for c in cases)
    done = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    lines = done.stdout.splitlines()
    assert len(lines) == len(cases), (len(lines), len(cases))
    return lines


def raw_call(L, base, c, stream):
    """One raw call of the entry point: every argument an explicit ctypes value.  Returns (rc, message)."""
    keep = []

    def ptr(v):
        return C.c_void_p(None if v["off"] is None else base + 8 * v["off"])

    def strides(v):
        if v["bs"] is None:
            return None
        keep.append((C.c_int64 * max(len(v["bs"]), 1))(*v["bs"]))
        return keep[-1]

    def view(v):
        if c["rank2"]:
            return [ptr(v), strides(v), C.c_int64(v["rst"]), C.c_size_t(v["len0"]), C.c_size_t(v["len1"])]
        return [ptr(v), strides(v), C.c_size_t(v["len1"])]

    op, var = c["op"], ([C.c_int(c["var"])] if c["rank2"] else [])
    if op in BINARY:
        args = view(c["x"]) + view(c["y"]) + (var if op in ("compose", "compose_adj") else []) + view(c["r"])
    elif op in SEEDED:
        args = view(c["x"]) + [ptr(c["y"]), strides(c["y"])] + view(c["r"])
    elif op == "pow":
        args = view(c["x"]) + [C.c_uint32(c["e"])] + view(c["r"])
    elif op == "evaluate_all_one":
        args = view(c["x"]) + [ptr(c["r"]), strides(c["r"])]
    else:
        args = view(c["x"]) + var + [C.c_size_t(c["k"])] + view(c["r"])
    batch = None if c["batch"] is None else (C.c_size_t * max(len(c["batch"]), 1))(*c["batch"])
    f = getattr(L, entry_name(c))
    f.restype = C.c_int
    rc = f(*args, batch, C.c_size_t(_nbatch(c)), C.c_void_p(stream))
    return rc, (L.gft_last_error() or b"").decode() if rc != 0 else None


def replay_c(cases, after=None):
    """Calls every case on the GPU; yields (case, rc, message).  `after` runs behind every call."""
    import torch

    import genfer_amd

    genfer_amd.init(0)
    L = genfer_amd.lib()
    buf = torch.zeros(BUFFER, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for c in cases:
        rc, msg = raw_call(L, buf.data_ptr(), c, stream)
        if after is not None:
            after(buf)
        yield c, rc, msg


# ---- the Python layer ------------------------------------------------------------------------------------------------------


# A case is a call of a public function: {"module", "fn", "args", "kwargs"}.  A tensor is {"t": shape} -- without storage, reporting
# a GPU placement -- with "dtype", "on" ("cpu": a real CPU tensor; "cuda:1": another GPU), "step" (the last axis strided) or "grad"
# where the case needs them; everything else (numbers, lists) is passed as it stands.


def T(*shape, **kw):
    return dict({"t": list(shape)}, **kw)


def python_cases():
    out = []

    def add(module, fn, *args, **kw):
        out.append({"module": module, "fn": fn, "args": list(args), "kwargs": kw})

    for mod, rank, planes, limit in (("series", 1, 0, 4096), ("interval_series", 1, 1, 2048), ("series2", 2, 0, 4096),
                                     ("interval_series2", 2, 1, 2048), ("series2_grad", 2, 0, 4096)):
        lead, it = [2] * planes, [8] if rank == 1 else [4, 8]
        X, S = T(*lead, 3, *it), T(*lead, 3)
        n_of = (lambda *v: v[-1]) if rank == 1 else (lambda *v: list(v))  # an order: an int at rank 1, a pair at rank 2
        vk = (lambda k: (k,)) if rank == 1 else (lambda k, var=1: (var, k))  # the observation ops' (var, k)
        big = [limit + 1] if rank == 1 else ([17, 241] if limit == 4096 else [2, 1025])
        less = it[:-1] + [7]
        if mod != "series2_grad":  # without an operand that requires grad, series2_grad IS series2
            # type, dtype, planes, axes: on the first operand, the second, the seeds and out
            add(mod, "mul", [1.0], X), add(mod, "mul", X, [1.0]), add(mod, "exp", X, seed=[1.0]), add(mod, "mul", X, X, out=[1.0])
            add(mod, "derivative", 1.0, *vk(1)), add(mod, "evaluate_all_one", X, out="o")
            f32 = dict(X, dtype="float32")
            add(mod, "mul", f32, X), add(mod, "div", X, f32), add(mod, "log", X, seed=dict(S, dtype="float32")), add(mod, "mul", X, X, out=f32)
            add(mod, "shift_down", f32, *vk(1)), add(mod, "evaluate_all_one", X, out=dict(S, dtype="float32"))
            if planes:
                add(mod, "mul", T(3, 3, *it), X), add(mod, "mul", X, T()), add(mod, "exp", X, seed=T(3)), add(mod, "mul", X, X, out=T(1, 3, *it))
                add(mod, "derivative", T(3, 3, *it), *vk(1)), add(mod, "evaluate_all_one", X, out=T(3))
            few = T(*lead, *it[1:])
            add(mod, "mul", few, X), add(mod, "mul", X, few), add(mod, "pow", X, 2, out=few), add(mod, "taylor_expansion_of_coeff", few, *vk(1))
            add(mod, "shift_down", X, *vk(1), out=few)
            strided, empty = dict(X, step=2), T(*lead, 3, *it[:-1], 0)
            add(mod, "mul", strided, X), add(mod, "compose", X, strided), add(mod, "mul", X, X, out=strided), add(mod, "derivative", strided, *vk(1))
            add(mod, "mul", empty, X), add(mod, "div", X, empty), add(mod, "exp", X, out=empty), add(mod, "evaluate_all_one", empty)
            if rank == 2:
                add(mod, "mul", T(*lead, 3, 0, 8), X)
            # the orders
            add(mod, "mul", X, X, n=n_of(4, 0)), add(mod, "exp", X, n=n_of(8, 0)), add(mod, "mul", X, X, n=n_of(*big)), add(mod, "pow", X, 2, n=n_of(*big))
            add(mod, "mul", X, X, n=n_of(4, 4)), add(mod, "mul", T(*lead, 3, *it[:-1], 4), X, n=n_of(4, 4)), add(mod, "log", X, n=n_of(4, 7))
            if rank == 2:
                add(mod, "mul", X, X, n=[2, 8]), add(mod, "mul", X, X, n=5), add(mod, "pow", X, 2, n=[1, 2, 3])
                add(mod, "compose", X, X, var=2), add(mod, "compose", X, X, True), add(mod, "derivative", X, 2, 1), add(mod, "shift_down", X, 0.0, 1)
            for e in (True, 1.5, -1, 2 ** 32):
                add(mod, "pow", X, e)
            # the observation ops: the limit, k, out
            add(mod, "derivative", T(*lead, 3, *big), *vk(1)), add(mod, "evaluate_all_one", T(*lead, *big))
            add(mod, "derivative", X, *vk(True)), add(mod, "taylor_expansion_of_coeff", X, *vk(1.5))
            for op in ("derivative", "taylor_expansion_of_coeff", "shift_down"):
                add(mod, op, X, *vk(8)), add(mod, op, X, *vk(-1))
            if rank == 2:
                add(mod, "derivative", X, 0, 4)
            add(mod, "derivative", X, *vk(1), out=X), add(mod, "shift_down", X, *vk(1), out=T(*lead, 2, *less))
            add(mod, "evaluate_all_one", X, out=T(*lead, 3, 1)), add(mod, "evaluate_all_one", X, out=T(*lead, 2))
            # out of the arithmetic ops
            add(mod, "mul", X, X, out=T(*lead, 3, *less)), add(mod, "mul", X, X, out=T(*lead, 1, *it)), add(mod, "exp", X, seed=S, out=T(*lead, *it))
            # the placement and the devices
            cpu, far = dict(X, on="cpu"), dict(X, on="cuda:1")
            add(mod, "mul", cpu, X), add(mod, "mul", X, cpu), add(mod, "exp", X, seed=dict(S, on="cpu")), add(mod, "mul", X, X, out=cpu)
            add(mod, "derivative", cpu, *vk(1)), add(mod, "evaluate_all_one", X, out=dict(S, on="cpu"))
            add(mod, "mul", X, far), add(mod, "log", X, seed=dict(S, on="cuda:1")), add(mod, "div", X, X, out=far)
            add(mod, "evaluate_all_one", X, out=dict(S, on="cuda:1"))
        G, SG = dict(X, grad=True), dict(S, grad=True)
        if mod in ("series", "series2_grad"):  # autograd: what cannot be differentiated, and the checks a Function's forward reaches
            add(mod, "exp", X, seed=SG), add(mod, "log", G, seed=SG), add(mod, "mul", G, X, out=X)
            add(mod, "compose", X, G, out=X), add(mod, "derivative", G, *vk(1), out=X), add(mod, "evaluate_all_one", G, out=S)
            add(mod, "mul", G, X, n=n_of(4, 4)), add(mod, "div", X, G, n=n_of(4, 0)), add(mod, "pow", G, -1), add(mod, "pow", G, 2, n=n_of(*big))
            add(mod, "mul", G, dict(X, on="cpu")), add(mod, "exp", G, seed=dict(S, on="cuda:1")), add(mod, "derivative", G, *vk(8))
            add(mod, "shift_down", dict(G, on="cpu"), *vk(1))
            if rank == 2:
                add(mod, "compose", G, X, var=2), add(mod, "derivative", G, 2, 1)
        elif mod != "interval_series":  # the raw modules refuse an operand that requires grad
            add(mod, "mul", G, X), add(mod, "div", X, G), add(mod, "exp", X, seed=SG), add(mod, "pow", G, 2), add(mod, "derivative", G, *vk(1))
            add(mod, "evaluate_all_one", G)
        else:  # interval_series: the observation ops do (its arithmetic ops run on the values: a finding, kept as it is)
            add(mod, "derivative", G, 1), add(mod, "evaluate_all_one", G)
        if mod in ("series", "series2"):  # the transposed operations: the result is the short side
            g = X
            long_ = T(3, *big)
            add(mod, "corr", g, g, n_of(4, 0)), add(mod, "corr", long_, g), add(mod, "corr", g, g, n_of(4, 9)), add(mod, "corr", g, T(3, *it[:-1], 9))
            av = () if rank == 1 else (1,)
            add(mod, "_compose_adj", g, g, *av, n_of(8, 0)), add(mod, "_compose_adj", long_, g, *av, n_of(4, 8))
            add(mod, "_compose_adj", g, g, *av, n_of(5, 8) if rank == 2 else 9), add(mod, "_compose_adj", g, T(3, *it[:-1], 9), *av, n_of(4, 8))
            add(mod, "corr", [1.0], g), add(mod, "corr", g, dict(g, on="cpu")), add(mod, "corr", g, g, out=T(3, *less))
            if rank == 2:
                add(mod, "corr", g, g, 5), add(mod, "_compose_adj", g, g, 2, [4, 8]), add(mod, "corr", g, T(3, 5, 8)), add(mod, "corr", g, g, [5, 8])
    return out


def _tensor(torch, spec):
    shape = list(spec["t"])
    step = spec.get("step", 1)
    shape[-1:] = [shape[-1] * step] if shape else []
    on = spec.get("on", "cuda:0")
    dtype = getattr(torch, spec.get("dtype", "float64"))
    if on == "cpu":
        t = torch.zeros(shape, dtype=dtype)
    else:  # no storage, and a placement on a GPU: every check in front of the library is reached without a device
        class Fake(torch.Tensor):
            @property
            def device(self):
                return torch.device(on)

        t = torch.zeros(shape, dtype=dtype, device="meta").as_subclass(Fake)
    if step > 1:
        t = t[..., ::step]
    return t.requires_grad_() if spec.get("grad") else t


def record_python():
    """Calls every case of python_cases(); each must be refused.  [{"case", "type", "message"}]"""
    import importlib

    import torch

    from genfer_amd import TaylorError

    out = []
    for c in python_cases():
        build = lambda a: _tensor(torch, a) if isinstance(a, dict) and "t" in a else a  # noqa: E731
        fn = getattr(importlib.import_module("genfer_amd." + c["module"]), c["fn"])
        try:
            fn(*(build(a) for a in c["args"]), **{k: build(v) for k, v in c["kwargs"].items()})
        except (TypeError, ValueError, TaylorError) as e:  # (anything else is no refusal of this layer: it propagates)
            out.append({"case": c, "type": type(e).__name__, "message": str(e)})
        else:
            raise AssertionError(f"accepted: {c}")
    return out


def load():
    if os.path.exists(TABLE):
        with open(TABLE) as f:
            return json.load(f)
    return {"python": [], "c": [], "accepted": []}


def main(argv):
    table = load()
    if argv[:1] == ["--c"]:
        table["c"] = []
        for c, rc, msg in replay_c(c_cases()):
            assert (rc, msg is None) in ((-1, False), (0, True)), (c, rc, msg)
            assert rc == -1 or 0 in (c["batch"] or []), f"a case was accepted and launched: {c}"
            table["c"].append({"case": c, "type": None if rc == 0 else "TaylorError", "message": msg})
    elif argv[:1] == ["--accepted"]:
        cases = accepted_cases()
        table["accepted"] = [{"case": c, "plan": line} for c, line in zip(cases, run_program(argv[1], cases))]
    elif argv[:1] == ["--python"]:
        table["python"] = record_python()
    else:
        sys.exit(__doc__)
    with open(argv[-1] if argv[-1].endswith(".json") else TABLE, "w") as f:  # one entry per line
        parts = [f' "{k}": [\n' + ",\n".join("  " + json.dumps(e) for e in v) + "\n ]" for k, v in table.items()]
        f.write("{\n" + ",\n".join(parts) + "\n}\n")
    print({k: len(v) for k, v in table.items()})


if __name__ == "__main__":
    sys.path.append(os.path.dirname(HERE))  # (behind PYTHONPATH: the table is recorded from the tree named there)
    main(sys.argv[1:])
