#!/usr/bin/env python3
"""Batched trivariate series (genfer_amd.series3) against the per-item loop through the handle API, on one GPU.

For each operation and each (B, n0, n1, n2) it times, between two events on torch's current stream after a warm-up,
  (a) the batched call, and
  (b) the per-item loop  from_torch(item) -> handle op -> to_torch(out[item])  on min(B, --loop-items) items, scaled to B
      (the only way to do this before the batched entry points existed),
and prints one JSON line per case: both times, their ratio, and the GMAC/s of the batched call (multiply-adds of the row
products, counted over the stored coefficients).  A summary line states the two standing targets of batched calls against the
loop measured in the same run: at least 10x for B >= 256, no slower than 1.1x for B < 256.

    python tools/bench_series3.py > profiles/r17/series3.json
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = "4096x4x4x4,65536x2x4x8,1024x8x8x8,256x16x16x16,64x8x8x64,1x16x16x16"
OPS = "mul,div,exp,log"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ops", default=OPS, help=f"comma-separated operations out of {OPS} (default: all)")
    ap.add_argument("--shapes", default=SHAPES, help=f"comma-separated BxN0xN1xN2 cases (default {SHAPES})")
    ap.add_argument("--loop-items", type=int, default=256, help="items the per-item loop is timed on (scaled to B)")
    ap.add_argument("--budget-ms", type=float, default=300.0, help="time each leg repeats for, roughly")
    ap.add_argument("--no-loop", action="store_true", help="skip leg (b)")
    args = ap.parse_args(argv)
    for op in args.ops.split(","):
        if op not in OPS.split(","):
            ap.error(f"unknown operation '{op}'")
    return args


def timed(torch, fn, budget_ms):
    """mean milliseconds per call: one warm-up, one probe, then as many repeats as the budget allows (at least 1)"""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    probe = a.elapsed_time(b)
    reps = int(max(1, min(200, budget_ms / max(probe, 1e-3))))
    if reps == 1:
        return probe, 1
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps, reps


def macs(n):
    """multiply-adds of the dense row products of one item: a triangle of terms on every axis"""
    return math.prod(k * (k + 1) / 2.0 for k in n)


def main(argv=None):
    args = parse_args(argv)
    import torch

    import genfer_amd
    from genfer_amd import series3

    genfer_amd.init(0)
    TP = genfer_amd.TaylorPoly
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(7)
    results = []
    for shape in args.shapes.split(","):
        B, *n = (int(t) for t in shape.lower().split("x"))
        N = math.prod(n)
        # bounded results at every order: a dominant constant term in the divisor, a small argument for exp
        x = (0.5 + torch.rand((B, *n), dtype=torch.float64, generator=gen) / N).to(dev)
        y = (0.5 + torch.rand((B, *n), dtype=torch.float64, generator=gen) / N).to(dev)
        y[:, 0, 0, 0] += 2.0
        out = torch.empty((B, *n), dtype=torch.float64, device=dev)
        for op in args.ops.split(","):
            seed = None
            if op in ("exp", "log"):
                seed = torch.tensor([getattr(math, op)(v) for v in x[:, 0, 0, 0].cpu().tolist()], dtype=torch.float64).to(dev)

            def batched():
                if op in ("mul", "div"):
                    getattr(series3, op)(x, y, out=out)
                else:
                    getattr(series3, op)(x, seed=seed, out=out)

            t_batch, reps_a = timed(torch, batched, args.budget_ms)
            items = min(B, args.loop_items)

            def loop():
                for b in range(items):
                    p = TP.from_torch(x[b])
                    if op == "mul":
                        r = p * TP.from_torch(y[b])
                    elif op == "div":
                        r = p / TP.from_torch(y[b])
                    else:
                        r = p.exp() if op == "exp" else p.log()
                    r.to_torch(out=out[b])

            rec = {"op": op, "B": B, "n0": n[0], "n1": n[1], "n2": n[2], "batched_ms": round(t_batch, 6), "batched_reps": reps_a,
                   "GMACps": round(B * macs(n) / (t_batch * 1e-3) / 1e9, 3)}
            if not args.no_loop:
                t_loop, reps_b = timed(torch, loop, args.budget_ms)
                t_loop *= B / items
                rec.update({"loop_ms": round(t_loop, 6), "loop_items": items, "loop_reps": reps_b, "loop_over_batched": round(t_loop / t_batch, 3)})
            results.append(rec)
            print(json.dumps(rec), flush=True)
    props = torch.cuda.get_device_properties(0)
    big = [r["loop_over_batched"] for r in results if r["B"] >= 256 and "loop_over_batched" in r]
    small = [r["loop_over_batched"] for r in results if r["B"] < 256 and "loop_over_batched" in r]
    print(json.dumps({"summary": True, "device": props.name, "cases": len(results),
                      "min_ratio_B_ge_256": min(big, default=None), "target_10x_met_B_ge_256": all(v >= 10.0 for v in big) if big else None,
                      "min_ratio_B_lt_256": min(small, default=None),
                      "target_no_slower_than_1.1x_met_B_lt_256": all(v >= 1 / 1.1 for v in small) if small else None}))


if __name__ == "__main__":
    main()
