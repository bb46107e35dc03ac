#!/usr/bin/env python3
"""The fused observation chain (observe_chain of genfer_amd.series / series2 and, with ``--interval``, of interval_series /
interval_series2) on one GPU, against the unfused sequence of this library's own batched calls.

One process.  Every case is warmed up on both legs first; then ``--rounds`` rounds, each timing both legs once between two events
on torch's current stream, the legs alternating within a round; a record holds the median over the rounds per leg with min and max.
The legs:
  fused    one ``observe_chain`` call, ``out=`` given: one launch;
  unfused  per step ``derivative(src, 1)``, ``mul(D[..., :d_t], [x, 1], n=d_t)`` and the scaling by the step's constant (torch's
           broadcast multiply for f64, ``mul`` by a one-coefficient series for intervals): three launches per step.  It computes
           the same polynomial through the general product (the same bits only where no path of mul_linear differs); a record
           holds the largest difference between the legs over the largest coefficient.
A shape is ``BxL`` (rank 1) or ``BxN0xN1`` (rank 2, both variables run); ``--steps`` are cut to the ``L - 2`` the axis allows.

    python tools/bench_series_observe_chain.py --out profiles/r23/series_observe_chain.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = "1x4096,65536x32,4096x256,1x64x64,65536x4x8"
SHAPES_IV = "1x2048,65536x32,4096x256,1x32x64,65536x4x8"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=None, help=f"comma-separated BxL (rank 1) or BxN0xN1 (rank 2) cases (default {SHAPES}; with --interval {SHAPES_IV})")
    ap.add_argument("--steps", default="4,32", help="comma-separated chain lengths, each cut to L - 2 (default 4,32)")
    ap.add_argument("--rounds", type=int, default=7, help="rounds; the medians are over them (default 7)")
    ap.add_argument("--reps", type=int, default=200, help="fused calls per timing (default 200)")
    ap.add_argument("--reps-unfused", type=int, default=10, help="unfused sequences per timing (default 10)")
    ap.add_argument("--interval", action="store_true", help="the Interval<F64> twins (interval_series, interval_series2) instead of f64")
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
    gen = torch.Generator(device="cpu").manual_seed(23)
    iv = args.interval
    lead = (2,) if iv else ()
    results = []

    def rand(*shape, lo=0.5):
        v = lo + torch.rand(shape, dtype=torch.float64, generator=gen)
        return (torch.stack([v, v * (1.0 + 1e-9)]) if iv else v).to(dev)

    for shape in (args.shapes or (SHAPES_IV if iv else SHAPES)).split(","):
        dims = [int(t) for t in shape.lower().split("x")]
        B, item = dims[0], tuple(dims[1:])
        rank = len(item)
        mod = (interval_series if iv else series) if rank == 1 else (interval_series2 if iv else series2)
        a = rand(B, *item)
        x = rand(B, lo=0.1)
        for var in ((None,) if rank == 1 else (0, 1)):
            ax = -1 if var is None else var - 2
            L = item[ax]
            va = () if rank == 1 else (var,)
            for want in sorted({min(int(s), L - 2) for s in args.steps.split(",")}):
                if want < 1:
                    continue
                n, d = want, L - want
                cs = rand(B, n, lo=0.25)
                other = () if rank == 1 else (min(item[1 + ax], d),)
                rshape = (d,) if rank == 1 else ((d,) + other if ax == -2 else other + (d,))
                out = torch.empty(lead + (B,) + rshape, dtype=torch.float64, device=dev)
                # the factor var(v, x): x + 1 * v, a two-coefficient series along the axis
                vs = torch.stack([x, torch.ones_like(x)], dim=-1)
                vs = vs if rank == 1 else (vs[..., None] if ax == -2 else vs[..., None, :])
                cone = cs[..., None] if rank == 1 else cs[..., None, None]  # [.., B, n, 1(, 1)]: step t is cone[..., t, :(, :)]

                def fused():
                    mod.observe_chain(a, *va, x, cs, d, out=out)

                def unfused():
                    src = a
                    for t in range(n):
                        dt = d + (n - 1 - t)
                        D = mod.derivative(src, *va, 1).narrow(ax, 0, dt)
                        if rank == 2:
                            D = D.narrow(-3 - ax, 0, min(D.shape[-3 - ax], dt))
                        nn = dt if rank == 1 else tuple(D.shape[-2:])
                        p = mod.mul(D, vs, n=nn)
                        src = mod.mul(p, cone[:, :, t] if iv else cone[:, t], n=nn) if iv else p * cone[:, t]
                    return src

                legs = {"fused": (fused, args.reps), "unfused": (unfused, args.reps_unfused)}
                for fn, _ in legs.values():
                    fn()
                    fn()
                # the two legs compute the same polynomial: the largest difference over the largest coefficient
                differ = float((unfused() - out).abs().max() / out.abs().max())
                torch.cuda.synchronize()
                times = {name: [] for name in legs}
                for _ in range(args.rounds):
                    for name, (fn, reps) in legs.items():
                        times[name].append(once(torch, fn, reps))
                med = {k: statistics.median(v) for k, v in times.items()}
                rec = {"element": "interval" if iv else "f64", "B": B, "item": list(item), "nsteps": n, "degree_p1": d}
                fused()
                rec["form"] = series.last_form()
                if var is not None:
                    rec["var"] = var
                for k, v in times.items():
                    rec.update({f"{k}_ms": round(med[k], 6), f"{k}_min_ms": round(min(v), 6), f"{k}_max_ms": round(max(v), 6)})
                rec.update({"unfused_over_fused": round(med["unfused"] / med["fused"], 3), "launches_unfused": 3 * n, "legs_differ_rel": differ, "rounds": args.rounds})
                results.append(rec)
                print(json.dumps(rec), flush=True)
    slower = [r for r in results if r["unfused_over_fused"] <= 1.0]
    summary = {"summary": True, "device": torch.cuda.get_device_properties(0).name, "cases": len(results),
               "min_unfused_over_fused": min((r["unfused_over_fused"] for r in results), default=None),
               "rows_where_fused_is_not_faster": [{k: r.get(k) for k in ("element", "B", "item", "var", "nsteps", "unfused_over_fused")} for r in slower]}
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results + [summary], fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
