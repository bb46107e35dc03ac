#!/usr/bin/env python3
"""Batched series (genfer_amd.series) against the per-row loop through the handle API, on one GPU.

For each operation and each (B, n) it times, between two events on torch's current stream after a warm-up,
  (a) the batched call, and
  (b) the per-row loop  from_torch(row) -> handle op -> to_torch(out[row])  on min(B, --loop-rows) rows, scaled to B
      (the only way to do this before the batched entry points existed),
and prints one JSON line per case: both times, their ratio, the algorithmic GB/s (8 * B * (nx + ny + n) bytes) and GMAC/s of
the batched call, and which form ran.  --form A|B asks for a form (dispatch thresholds are set from such sweeps).

    python tools/bench_series.py > profiles/r07/series_batch.json
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = "4096x16,4096x64,65536x32,1024x256,64x1024,1x4096"
OPS = "mul,div,exp,log"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ops", default=OPS, help=f"comma-separated operations (default {OPS})")
    ap.add_argument("--shapes", default=SHAPES, help=f"comma-separated BxN cases (default {SHAPES})")
    ap.add_argument("--form", choices=["auto", "A", "B"], default="auto", help="ask the library for a form (default: its thresholds)")
    ap.add_argument("--loop-rows", type=int, default=256, help="rows the per-row loop is timed on (scaled to B)")
    ap.add_argument("--budget-ms", type=float, default=300.0, help="time each leg repeats for, roughly")
    ap.add_argument("--no-loop", action="store_true", help="skip leg (b)")
    return ap.parse_args(argv)


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


def main(argv=None):
    args = parse_args(argv)
    import torch

    import genfer_amd
    from genfer_amd import series

    genfer_amd.init(0)
    TP = genfer_amd.TaylorPoly
    dev = torch.device("cuda", 0)
    series.set_form(None if args.form == "auto" else args.form)
    gen = torch.Generator(device="cpu").manual_seed(7)
    results = []
    for shape in args.shapes.split(","):
        B, n = (int(t) for t in shape.lower().split("x"))
        # bounded results at every order: a dominant constant term in the divisor, a small argument for exp
        x = (0.5 + torch.rand((B, n), dtype=torch.float64, generator=gen) / n).to(dev)
        y = (0.5 + torch.rand((B, n), dtype=torch.float64, generator=gen) / n).to(dev)
        y[:, 0] += 2.0
        out = torch.empty((B, n), dtype=torch.float64, device=dev)
        for op in args.ops.split(","):
            seed = None
            if op in ("exp", "log"):
                seed = torch.tensor([getattr(math, op)(v) for v in x[:, 0].cpu().tolist()], dtype=torch.float64).to(dev)

            def batched():
                if op in ("mul", "div"):
                    getattr(series, op)(x, y, out=out)
                else:
                    getattr(series, op)(x, seed=seed, out=out)

            t_batch, reps_a = timed(torch, batched, args.budget_ms)
            form = series.last_form()
            rows = min(B, args.loop_rows)

            def loop():
                for b in range(rows):
                    p = TP.from_torch(x[b])
                    if op == "mul":
                        r = p * TP.from_torch(y[b])
                    elif op == "div":
                        r = p / TP.from_torch(y[b])
                    else:
                        r = p.exp() if op == "exp" else p.log()
                    r.to_torch(out=out[b])

            rec = {"op": op, "B": B, "n": n, "form": form, "batched_ms": round(t_batch, 6), "batched_reps": reps_a}
            macs = B * n * (n + 1) / 2.0
            nbytes = 8.0 * B * (n + (n if op in ("mul", "div") else 0) + n)
            rec["algorithmic_GBps"] = round(nbytes / (t_batch * 1e-3) / 1e9, 3)
            rec["GMACps"] = round(macs / (t_batch * 1e-3) / 1e9, 3)
            if not args.no_loop:
                t_loop, reps_b = timed(torch, loop, args.budget_ms)
                t_loop *= B / rows
                rec.update({"loop_ms": round(t_loop, 6), "loop_rows": rows, "loop_reps": reps_b, "loop_over_batched": round(t_loop / t_batch, 3)})
            results.append(rec)
            print(json.dumps(rec), flush=True)
    series.set_form(None)
    props = torch.cuda.get_device_properties(0)
    print(json.dumps({"summary": True, "device": props.name, "asked_form": args.form, "cases": len(results),
                      "min_ratio_B_ge_256": min([r["loop_over_batched"] for r in results if r["B"] >= 256 and "loop_over_batched" in r], default=None),
                      "min_ratio_B_lt_256": min([r["loop_over_batched"] for r in results if r["B"] < 256 and "loop_over_batched" in r], default=None)}))


if __name__ == "__main__":
    main()
