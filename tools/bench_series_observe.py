#!/usr/bin/env python3
"""The batched observation ops (derivative, taylor_expansion_of_coeff, shift_down, evaluate_all_one of genfer_amd.series and
genfer_amd.series2) on one GPU, against the two ways to take these steps without them.

One process.  Every (shape, op) is warmed up on every leg first; then ``--rounds`` rounds, each timing every leg once between two
events on torch's current stream (``--reps`` calls per timing), the legs alternating within a round; the record holds the median
over the rounds per leg and the spread (max - min) / median of the batched leg and of the torch leg.  ``k`` is half the axis; at
rank 2 both variables run.  The legs:
  (a) the batched call, ``out=`` given;
  (b) the per-item loop  from_torch(item) -> handle op -> to_torch(out[item])  on min(B, --loop-items) items, scaled to B.  The handle
      API has no evaluate_all_one: its loop is shift_down by len - 1 on every axis (the mass read-out as a handle user takes it);
  (c) the torch formulation a caller could write: ``x[..., k:] * table`` for the scalings (the table taken from the batched op on
      ones), ``cat(head.sum + x[k], tail)`` for shift_down, ``x.sum`` for evaluate_all_one.  The sums have torch's order, not the
      reference's: a yardstick for speed only.
Each record also has the algorithmic bytes (operand elements read once, result written once) over the batched time in GB/s and its
share of 8 TB/s.  The summary states the standing targets against (b) -- at least 10x for B >= 256, no slower than 1.1x below -- and
for (c) the cases where the batched call is slower than the torch leg by more than the larger spread of the two.

    python tools/bench_series_observe.py --out profiles/r15/series_observe.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = "65536x32,4096x64,1024x256,64x1024,4096x8x8,1024x16x16,256x64x64"
OPS = "derivative,taylor_expansion_of_coeff,shift_down,evaluate_all_one"
PEAK_GBPS = 8000.0


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ops", default=OPS, help=f"comma-separated operations (default: {OPS})")
    ap.add_argument("--shapes", default=SHAPES, help=f"comma-separated BxN (rank 1) or BxN0xN1 (rank 2) cases (default {SHAPES})")
    ap.add_argument("--rounds", type=int, default=7, help="rounds; the medians are over them (default 7)")
    ap.add_argument("--reps", type=int, default=20, help="calls per timing of legs (a) and (c) (default 20)")
    ap.add_argument("--loop-items", type=int, default=256, help="items the per-item loop is timed on (scaled to B)")
    ap.add_argument("--no-loop", action="store_true", help="skip leg (b)")
    ap.add_argument("--out", default=None, help="also write the records as a JSON list to this file")
    args = ap.parse_args(argv)
    for op in args.ops.split(","):
        if op not in OPS.split(","):
            ap.error(f"unknown operation '{op}'")
    return args


def once(torch, fn, reps):
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
    from genfer_amd import series, series2

    genfer_amd.init(0)
    TP = genfer_amd.TaylorPoly
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(15)
    results = []
    for shape in args.shapes.split(","):
        dims = [int(t) for t in shape.lower().split("x")]
        B, item = dims[0], tuple(dims[1:])
        rank = len(item)
        mod = series if rank == 1 else series2
        x = (0.5 + torch.rand((B,) + item, dtype=torch.float64, generator=gen)).to(dev)
        per = item[0] * item[-1] if rank == 2 else item[0]
        for op in args.ops.split(","):
            ev = op == "evaluate_all_one"
            for var in ((None,) if rank == 1 or ev else (0, 1)):
                ax = -1 if var is None else var - 2
                ln = item[ax]
                k = ln // 2
                va = () if rank == 1 else (var,)
                oshape = list(item)
                oshape[ax] = ln - k
                out = torch.empty((B,) if ev else (B,) + tuple(oshape), dtype=torch.float64, device=dev)
                items = min(B, args.loop_items)
                if ev:
                    def batched():
                        mod.evaluate_all_one(x, out=out)

                    def written():
                        return torch.sum(x, dim=tuple(range(1, 1 + rank)), out=out)

                    def loop():
                        for b in range(items):
                            p = TP.from_torch(x[b])
                            for v in range(rank - 1, -1, -1):
                                p = p.shift_down(v, item[v] - 1)
                            p.to_torch(out=out[b].reshape((1,) * rank))
                    moved = 8.0 * B * (per + 1)
                else:
                    f = getattr(mod, op)
                    hv = 0 if rank == 1 else var
                    if op == "shift_down":
                        def written():
                            xl = x.movedim(ax, -1)
                            head = xl[..., :k].sum(-1, keepdim=True) + xl[..., k:k + 1]
                            return torch.cat([head, xl[..., k + 1:]], dim=-1).movedim(-1, ax)
                        moved = 8.0 * B * (per + per // ln * (ln - k))
                    else:
                        tab = getattr(series, op)(torch.ones(ln, dtype=torch.float64, device=dev), k)
                        tab = tab if ax == -1 else tab[:, None]

                        def written():
                            return torch.mul(x.narrow(ax, k, ln - k), tab, out=out)
                        moved = 8.0 * B * 2 * (per // ln * (ln - k))

                    def batched():
                        f(x, *va, k, out=out)

                    def loop():
                        for b in range(items):
                            getattr(TP.from_torch(x[b]), op)(hv, k).to_torch(out=out[b])
                legs = {"batched": (batched, args.reps), "torch": (written, args.reps)}
                if not args.no_loop:
                    legs["loop"] = (loop, 1)
                for fn, _ in legs.values():  # warm every leg of the shape before any is timed
                    fn()
                    fn()
                torch.cuda.synchronize()
                times = {name: [] for name in legs}
                for _ in range(args.rounds):
                    for name, (fn, reps) in legs.items():
                        times[name].append(once(torch, fn, reps))
                med = {name: statistics.median(v) for name, v in times.items()}
                spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
                rec = {"op": op, "B": B, "item": list(item), "k": None if ev else k, "batched_ms": round(med["batched"], 6),
                       "batched_spread": round(spread["batched"], 3), "torch_ms": round(med["torch"], 6), "torch_spread": round(spread["torch"], 3),
                       "torch_over_batched": round(med["torch"] / med["batched"], 3), "GBps": round(moved / (med["batched"] * 1e-3) / 1e9, 2),
                       "share_of_8TBps": round(moved / (med["batched"] * 1e-3) / 1e9 / PEAK_GBPS, 4), "rounds": args.rounds, "reps": args.reps}
                if var is not None:
                    rec["var"] = var
                if "loop" in med:
                    t_loop = med["loop"] * B / items
                    rec.update({"loop_ms": round(t_loop, 6), "loop_items": items, "loop_over_batched": round(t_loop / med["batched"], 3)})
                results.append(rec)
                print(json.dumps(rec), flush=True)
    big = [r["loop_over_batched"] for r in results if r["B"] >= 256 and "loop_over_batched" in r]
    small = [r["loop_over_batched"] for r in results if r["B"] < 256 and "loop_over_batched" in r]
    slower = [{"op": r["op"], "B": r["B"], "item": r["item"], "var": r.get("var"), "torch_over_batched": r["torch_over_batched"]}
              for r in results if r["torch_over_batched"] < 1.0 - max(r["batched_spread"], r["torch_spread"])]
    summary = {"summary": True, "device": torch.cuda.get_device_properties(0).name, "cases": len(results),
               "min_ratio_B_ge_256": min(big, default=None), "target_10x_met_B_ge_256": all(v >= 10.0 for v in big) if big else None,
               "min_ratio_B_lt_256": min(small, default=None), "target_no_slower_than_1.1x_met_B_lt_256": all(v >= 1 / 1.1 for v in small) if small else None,
               "slower_than_torch_beyond_spread": slower}
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results + [summary], fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
