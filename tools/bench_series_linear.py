#!/usr/bin/env python3
"""The batched affine substitution compose_linear (genfer_amd.series / series2 and the interval twins) on one GPU, against this
library's own two spellings of the same polynomial.

One process.  Every leg of a case runs once (that call sizes its repetitions) and once more to warm up; then ``--rounds`` rounds,
each timing every leg once between two events on torch's current stream, the legs alternating within a round; a record holds the
median over the rounds per leg with min and max.
The legs:
  fused    one ``compose_linear`` call, ``out=`` given: one launch, about nf * n multiply-adds per item;
  compose  ``compose(f, [c, m])``: the general substitution, Horner's loop with the general product at every step (other bits,
           about nf * n^2 / 2 multiply-adds per item, on one workgroup);
  loop     Horner's loop in Python, per step one ``mul_linear`` call and the slice added by torch: two launches per step (over
           intervals torch adds the bounds without widening: the same launches, not the same bits).
The repetitions of a timing are sized from a leg's first call so that one timing takes about ``--ms`` milliseconds (at least one
call); a leg whose first call takes longer than ``--skip-above`` seconds is not run again: that call is its one round, and the
record says so (``<leg>_rounds``).  A row is ``BxL`` (rank 1) or ``BxN0xN1`` (rank 2, every (var, wvar) runs); ``nf`` is 4 and the
full length on the replaced variable.

    python tools/bench_series_linear.py --out profiles/r24/series_linear.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = "1x4096,65536x32,4096x256,1x64x64,65536x4x8"
ROWS_IV = "1x2048,65536x32,4096x256,1x32x64,65536x4x8"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default=None, help=f"comma-separated BxL (rank 1) or BxN0xN1 (rank 2) cases (default {ROWS}; intervals {ROWS_IV})")
    ap.add_argument("--elements", default="f64,interval", help="comma-separated: f64, interval (default both)")
    ap.add_argument("--nf", default="4,full", help="comma-separated lengths of f on the replaced variable: integers or 'full' (default 4,full)")
    ap.add_argument("--rounds", type=int, default=7, help="rounds; the medians are over them (default 7)")
    ap.add_argument("--ms", type=float, default=20.0, help="the time one timing aims at, in milliseconds (default 20)")
    ap.add_argument("--skip-above", type=float, default=1.0, help="a leg whose single call takes longer (seconds) is timed in one round (default 1)")
    ap.add_argument("--out", default=None, help="also write the records as a JSON list to this file")
    return ap.parse_args(argv)


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
    from genfer_amd import interval_series, interval_series2, series, series2

    genfer_amd.init(0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(24)
    results = []
    for element in args.elements.split(","):
        iv = element == "interval"
        lead = (2,) if iv else ()

        def rand(*shape, lo=-0.5, width=1.0):
            v = lo + width * torch.rand(shape, dtype=torch.float64, generator=gen)
            return (torch.stack([v, v + 1e-9 * v.abs()]) if iv else v).to(dev)

        for row in (args.rows or (ROWS_IV if iv else ROWS)).split(","):
            dims = [int(t) for t in row.lower().split("x")]
            B, n = dims[0], tuple(dims[1:])
            rank = len(n)
            mod = (interval_series if iv else series) if rank == 1 else (interval_series2 if iv else series2)
            c, m = rand(B, lo=0.05, width=0.1), rand(B, lo=0.85, width=0.1)  # (c + m < 1: the Horner sums stay bounded)
            for v, w in (((0, 0),) if rank == 1 else ((0, 0), (1, 1), (0, 1), (1, 0))):
                for want in args.nf.split(","):
                    # f fills the result on the replaced variable (w == v), or is as long as the orders leave room for (w != v)
                    nfv = n[v] if want == "full" else min(int(want), n[v])
                    item = list(n)
                    item[v] = nfv
                    if w != v:
                        item[w] = max(1, n[w] - nfv + 1)
                    item = tuple(item)
                    f = rand(B, *item)
                    out = torch.empty(lead + (B,) + n, dtype=torch.float64, device=dev)
                    va, ax_v, ax_w = (() if rank == 1 else (v,)), v - rank, w - rank
                    g = torch.stack([c, m], dim=-1)  # the affine series [c, m] along axis w
                    g = g if rank == 1 else (g[..., None] if w == 0 else g[..., None, :])
                    nn = n[0] if rank == 1 else n
                    slen = item[w] if w != v else 1

                    def fused():
                        if rank == 1:
                            return mod.compose_linear(f, c, m, n=nn, out=out)
                        return mod.compose_linear(f, v, c, m, wvar=w, n=nn, out=out)

                    def compose():
                        return mod.compose(f, g, *va, n=nn)

                    def loop():
                        res = f.narrow(ax_v, nfv - 1, 1)
                        for i in range(nfv - 2, -1, -1):
                            shape = list(res.shape[-rank:])
                            shape[w] = min(n[w], shape[w] + 1)
                            res = mod.mul_linear(res, *(() if rank == 1 else (w,)), c, m, n=shape[0] if rank == 1 else tuple(shape))
                            res.narrow(ax_w, 0, slen).add_(f.narrow(ax_v, i, 1))  # (over intervals: the bounds' sums, not widened)
                        return res

                    legs = {"fused": fused, "compose": compose, "loop": loop}
                    reps, times, first = {}, {}, {}
                    for name, fn in legs.items():  # the first call: it sizes the repetitions, and its result is compared below
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record()
                        first[name] = fn()
                        t1.record()
                        t1.synchronize()
                        single = t0.elapsed_time(t1)
                        slow = single > 1e3 * args.skip_above
                        reps[name] = 0 if slow else max(1, int(args.ms / max(single, 1e-3)))
                        times[name] = [single] if slow else []
                    # the legs compute the same polynomial: the largest difference over the largest coefficient
                    scale = float(out.abs().max())
                    block = lambda t: tuple(slice(0, k) for k in t.shape)  # noqa: E731
                    differ = {k: float((first[k] - out[block(first[k])]).abs().max() / scale) for k in ("compose", "loop")}
                    for name, fn in legs.items():
                        if reps[name]:
                            once(torch, fn, reps[name])  # warm
                    for _ in range(args.rounds):
                        for name, fn in legs.items():
                            if reps[name]:
                                times[name].append(once(torch, fn, reps[name]))
                    med = {k: statistics.median(t) for k, t in times.items()}
                    rec = {"element": element, "B": B, "n": list(n), "f": list(item), "nf": nfv}
                    if rank == 2:
                        rec.update({"var": v, "wvar": w})
                    fused()
                    rec["form"] = series.last_form()
                    for k, t in times.items():
                        rec.update({f"{k}_ms": round(med[k], 6), f"{k}_min_ms": round(min(t), 6), f"{k}_max_ms": round(max(t), 6), f"{k}_rounds": len(t)})
                    rec.update({"compose_over_fused": round(med["compose"] / med["fused"], 3), "loop_over_fused": round(med["loop"] / med["fused"], 3),
                                "launches_loop": 2 * (nfv - 1), "legs_differ_rel": differ})
                    results.append(rec)
                    print(json.dumps(rec), flush=True)
    slower = [r for r in results if min(r["compose_over_fused"], r["loop_over_fused"]) <= 1.0]
    summary = {"summary": True, "device": torch.cuda.get_device_properties(0).name, "cases": len(results),
               "min_compose_over_fused": min((r["compose_over_fused"] for r in results), default=None),
               "min_loop_over_fused": min((r["loop_over_fused"] for r in results), default=None),
               "rows_where_fused_is_not_faster": [{k: r.get(k) for k in ("element", "B", "n", "var", "wvar", "nf", "compose_over_fused", "loop_over_fused")}
                                                  for r in slower]}
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results + [summary], fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
