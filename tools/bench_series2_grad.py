#!/usr/bin/env python3
"""The transposed bivariate operations (genfer_amd.series2.corr / _compose_adj) against the formulations they replace, on one GPU.

corr        series2.corr(g, y) against  flip -> series2.mul -> flip -> slice  (the same multiply-adds and two copies more)
adj         series2._compose_adj(gh, g, var, nf) against the unfused loop of S - 1 series2.corr calls at the compact shapes L_i, for
            both variables
backward    forward + backward of every operation of genfer_amd.series2_grad, beside the forward pass alone

The two legs of a comparison alternate within the run: ``--rounds`` rounds, each timing leg A and then leg B between two events on
torch's current stream over as many repeats as ``--budget-ms`` allows, after a warm-up of both.  A record holds the median of the
rounds and the spread (min, max) of each leg.  ``--lib PATH`` loads another build of libgftaylor.so (a lane-count variant).

    python tools/bench_series2_grad.py > profiles/r14/series2_grad.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OPS = "corr,adj,backward"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ops", default=OPS, help=f"comma-separated out of {OPS} (default: all)")
    ap.add_argument("--corr-shapes", default="256x32x32,256x64x64", help="BxG0xG1 cases of corr")
    ap.add_argument("--adj-shapes", default="256x32x32", help="BxN0xN1 cases of adj and backward: f, g and n all of that shape")
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds per comparison (default 7)")
    ap.add_argument("--budget-ms", type=float, default=200.0, help="time one leg of one round repeats for, roughly")
    ap.add_argument("--lib", default=None, help="another build of libgftaylor.so to load")
    ap.add_argument("--tag", default=None, help="a label copied into every record")
    args = ap.parse_args(argv)
    for op in args.ops.split(","):
        if op not in OPS.split(","):
            ap.error(f"unknown operation '{op}'")
    return args


def reps_for(torch, fn, budget_ms):
    fn()  # warm-up
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return int(max(1, min(1000, budget_ms / max(a.elapsed_time(b), 1e-3))))


def once(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def compare(torch, legs, rounds, budget_ms):
    """legs: {name: fn}.  Alternates the legs for `rounds` rounds; {name: {"ms": median, "min": .., "max": .., "reps": ..}}"""
    reps = {k: reps_for(torch, fn, budget_ms) for k, fn in legs.items()}
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(once(torch, fn, reps[k]))
    return {k: {"ms": round(statistics.median(v), 6), "min": round(min(v), 6), "max": round(max(v), 6), "reps": reps[k]} for k, v in times.items()}


def compact_shapes(nf, ng, n, var):
    S, ln = (nf[0], nf[1]) if var == 0 else (nf[1], nf[0])
    base = (1, ln) if var == 0 else (ln, 1)
    return [tuple(min(base[a] + (S - 1 - i) * (ng[a] - 1), n[a]) for a in (0, 1)) for i in range(S)]


def unfused_adj(torch, series2, gh, g, var, nf):
    """_compose_adj before it had a kernel: S - 1 series2.corr calls at the compact shapes, a slice collected from each"""
    L = compact_shapes(nf, tuple(g.shape[-2:]), tuple(gh.shape[-2:]), var)
    ln = nf[1] if var == 0 else nf[0]
    a = gh[..., :L[0][0], :L[0][1]]
    out = []
    for i in range(len(L)):
        out.append(a[..., 0, :ln] if var == 0 else a[..., :ln, 0])
        if i + 1 < len(L):
            a = series2.corr(a, g, L[i + 1])
    return torch.stack(out, dim=-2 if var == 0 else -1)


def main(argv=None):
    args = parse_args(argv)
    import torch

    import genfer_amd

    if args.lib:
        genfer_amd.LIB_PATH = os.path.abspath(args.lib)
    from genfer_amd import series2, series2_grad

    genfer_amd.init(0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(11)
    ops = args.ops.split(",")
    tag = {"tag": args.tag} if args.tag else {}
    results = []

    def rand(shape, scale=1.0):
        return (0.5 + torch.rand(shape, dtype=torch.float64, generator=gen) * scale).to(dev)

    def emit(rec):
        results.append(rec)
        print(json.dumps({**tag, **rec}), flush=True)

    if "corr" in ops:
        for shape in args.corr_shapes.split(","):
            B, g0, g1 = (int(t) for t in shape.lower().split("x"))
            g, y = rand((B, g0, g1)), rand((B, g0, g1))
            out = torch.empty_like(g)
            flips = lambda: torch.flip(series2.mul(torch.flip(g, (-2, -1)), y, n=(g0, g1)), (-2, -1))[..., :g0, :g1]  # noqa: E731
            assert torch.equal(series2.corr(g, y), flips())
            t = compare(torch, {"corr": lambda: series2.corr(g, y, out=out), "flip_mul_flip": flips, "mul": lambda: series2.mul(g, y, out=out)},
                        args.rounds, args.budget_ms)
            emit({"op": "corr", "B": B, "g0": g0, "g1": g1, **t, "flip_over_corr": round(t["flip_mul_flip"]["ms"] / t["corr"]["ms"], 3),
                  "corr_over_mul": round(t["corr"]["ms"] / t["mul"]["ms"], 3)})
    for shape in args.adj_shapes.split(","):
        B, n0, n1 = (int(t) for t in shape.lower().split("x"))
        n = (n0, n1)
        if "adj" in ops:
            gh, g = rand((B,) + n), rand((B,) + n, 1.0 / (n0 * n1))
            for var in (0, 1):
                assert torch.equal(series2._compose_adj(gh, g, var, n), unfused_adj(torch, series2, gh, g, var, n))
                out = torch.empty((B,) + n, dtype=torch.float64, device=dev)
                t = compare(torch, {"adj": lambda: series2._compose_adj(gh, g, var, n, out=out), "chain": lambda: unfused_adj(torch, series2, gh, g, var, n)},
                            args.rounds, args.budget_ms)
                emit({"op": "adj", "var": var, "B": B, "n0": n0, "n1": n1, **t, "chain_over_adj": round(t["chain"]["ms"] / t["adj"]["ms"], 3)})
        if "backward" in ops:
            x, y = rand((B,) + n, 1.0 / (n0 * n1)), rand((B,) + n, 1.0 / (n0 * n1))
            y[:, 0, 0] += 2.0
            gz = rand((B,) + n)
            cases = [("mul", lambda a, b: series2_grad.mul(a, b), True), ("div", lambda a, b: series2_grad.div(a, b), True),
                     ("exp", lambda a, b: series2_grad.exp(a), False), ("log", lambda a, b: series2_grad.log(a), False),
                     ("pow", lambda a, b: series2_grad.pow(a, 5), False), ("compose0", lambda a, b: series2_grad.compose(a, b, 0), True),
                     ("compose1", lambda a, b: series2_grad.compose(a, b, 1), True)]
            for name, fn, binary in cases:
                xt, yt = x.clone().requires_grad_(), y.clone().requires_grad_(binary)

                def both():
                    xt.grad = yt.grad = None
                    fn(xt, yt).backward(gz)

                def forward():
                    with torch.no_grad():
                        fn(xt, yt)

                t = compare(torch, {"forward": forward, "forward_backward": both}, args.rounds, args.budget_ms)
                emit({"op": "backward", "of": name, "B": B, "n0": n0, "n1": n1, **t,
                      "backward_over_forward": round((t["forward_backward"]["ms"] - t["forward"]["ms"]) / t["forward"]["ms"], 3)})
    corr = [r["flip_over_corr"] for r in results if r["op"] == "corr"]
    adj = [r["chain_over_adj"] for r in results if r["op"] == "adj"]
    print(json.dumps({**tag, "summary": True, "device": torch.cuda.get_device_properties(0).name, "cases": len(results),
                      "min_flip_over_corr": min(corr, default=None), "corr_no_slower_than_flip_mul_flip": all(v >= 1.0 for v in corr) if corr else None,
                      "min_chain_over_adj": min(adj, default=None), "compose_adj_no_slower_than_chain": all(v >= 1.0 for v in adj) if adj else None}))


if __name__ == "__main__":
    main()
