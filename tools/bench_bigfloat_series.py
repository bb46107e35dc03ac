#!/usr/bin/env python3
"""Batched BigFloat series (genfer_amd.bigfloat_series) against the two other element types of the same layer, on one GPU.

For each of the six operations and each (B, n) of tools/bench_series.py --interval's shapes it times three legs on the same shapes:
  (big) bigfloat_series on [2, B, n] = (factor, exponent) tensors, the encoded operands,
  (a)   interval_series on [2, B, n] = (lo, hi) tensors -- the same planes and the same LDS footprint, a different element, and
  (b)   the float64 series call on the decoded values [B, n].
Every leg is warmed, then the legs take turns for --rounds rounds (big, a, b, big, a, b, ...), a round of a leg being --reps calls
between two events on torch's current stream; a record holds each leg's median over the rounds with its spread (min and max), the
two ratios big / a and big / b of the medians, and the form that ran.  Both ratios are reported, not judged.

compose runs with nf = ng = min(n, --compose-m) (the whole Horner loop of an item is one workgroup's), pow raises to --pow-e; exp and
log are handed their seeds.

    python tools/bench_bigfloat_series.py > profiles/r25/bigfloat_series.json
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = "4096x16,4096x64,65536x32,1024x256,64x1024,1x2048"  # bench_series.py's, n capped at 2048 as --interval caps it
OPS = "mul,div,exp,log,compose,pow"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ops", default=OPS, help=f"comma-separated operations (default {OPS})")
    ap.add_argument("--shapes", default=SHAPES, help=f"comma-separated BxN cases (default {SHAPES})")
    ap.add_argument("--pow-e", type=int, default=5, help="the exponent of pow (default 5)")
    ap.add_argument("--compose-m", type=int, default=64, help="nf = ng = min(n, this) for compose (default 64)")
    ap.add_argument("--rounds", type=int, default=7, help="rounds per leg, the legs alternating (default 7)")
    ap.add_argument("--reps", type=int, default=0, help="calls per round (default: sized so that a round takes about --round-ms)")
    ap.add_argument("--round-ms", type=float, default=40.0, help="the time a round of a leg is sized to (default 40)")
    args = ap.parse_args(argv)
    for op in args.ops.split(","):
        if op not in OPS.split(","):
            ap.error(f"unknown operation '{op}'")
    return args


def one_round(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main(argv=None):
    args = parse_args(argv)
    import torch

    import genfer_amd
    from genfer_amd import bigfloat_series as bfs
    from genfer_amd import interval_series as ivs
    from genfer_amd import series

    genfer_amd.init(0)
    dev = torch.device("cuda", 0)
    series.set_form(None)
    gen = torch.Generator(device="cpu").manual_seed(7)
    results = []
    for shape in args.shapes.split(","):
        B, n = (int(t) for t in shape.lower().split("x"))
        n = min(n, 2048)
        m = min(n, args.compose_m)
        # bench_series.py's data -- bounded results at every order: a dominant constant term in the divisor, a small argument for exp
        x = (0.5 + torch.rand((B, n), dtype=torch.float64, generator=gen) / n).to(dev)
        y = (0.5 + torch.rand((B, n), dtype=torch.float64, generator=gen) / n).to(dev)
        y[:, 0] += 2.0
        operands = {"big": (bfs, bfs.encode(x), bfs.encode(y)),
                    "interval": (ivs, torch.stack([x, x * (1.0 + 2.0**-30)]), torch.stack([y, y * (1.0 + 2.0**-30)])),
                    "f64": (series, bfs.decode(bfs.encode(x)), bfs.decode(bfs.encode(y)))}
        outs = {k: torch.empty_like(v[1]) for k, v in operands.items()}
        for op in args.ops.split(","):
            legs, forms = {}, {}
            for leg, (mod, xx, yy) in operands.items():
                seed = None
                if op in ("exp", "log"):  # the values' own exp / log (intervals: unwidened; BigFloat: encoded) -- timing only
                    s = torch.tensor([getattr(math, op)(v) for v in x[:, 0].cpu().tolist()], dtype=torch.float64).to(dev)
                    seed = {"big": lambda: bfs.encode(s), "interval": lambda: torch.stack([s, s]), "f64": lambda: s}[leg]()
                out = outs[leg]

                def call(mod=mod, xx=xx, yy=yy, seed=seed, out=out):
                    if op in ("mul", "div"):
                        getattr(mod, op)(xx, yy, out=out)
                    elif op == "compose":
                        mod.compose(xx[..., :m], yy[..., :m], n=n, out=out)
                    elif op == "pow":
                        mod.pow(xx, args.pow_e, out=out)
                    else:
                        getattr(mod, op)(xx, seed=seed, out=out)

                legs[leg] = call
            reps = {}
            for leg, call in legs.items():  # warm every leg, and size its rounds
                call()
                torch.cuda.synchronize()
                probe = one_round(torch, call, 1)
                forms[leg] = series.last_form()
                reps[leg] = args.reps or int(max(1, min(200, args.round_ms / max(probe, 1e-3))))
            times = {leg: [] for leg in legs}
            for _ in range(args.rounds):
                for leg, call in legs.items():
                    times[leg].append(one_round(torch, call, reps[leg]))
            med = {leg: statistics.median(t) for leg, t in times.items()}
            rec = {"op": op, "B": B, "n": n, "rounds": args.rounds}
            if op == "compose":
                rec["nf"] = rec["ng"] = m
            if op == "pow":
                rec["e"] = args.pow_e
            for leg in legs:
                rec[leg] = {"ms": round(med[leg], 6), "min_ms": round(min(times[leg]), 6), "max_ms": round(max(times[leg]), 6),
                            "reps": reps[leg], "form": forms[leg]}
            rec["big_over_interval"] = round(med["big"] / med["interval"], 3)
            rec["big_over_f64"] = round(med["big"] / med["f64"], 3)
            results.append(rec)
            print(json.dumps(rec), flush=True)
    props = torch.cuda.get_device_properties(0)
    oi, of = [r["big_over_interval"] for r in results], [r["big_over_f64"] for r in results]
    print(json.dumps({"summary": True, "device": props.name, "cases": len(results), "rounds": args.rounds,
                      "big_over_interval_min_median_max": [min(oi), statistics.median(oi), max(oi)] if oi else None,
                      "big_over_f64_min_median_max": [min(of), statistics.median(of), max(of)] if of else None}))


if __name__ == "__main__":
    main()
