#!/usr/bin/env python3
"""The fused negative-binomial observation (observe_negbinomial of genfer_amd.series / series2 and, with ``--interval``, of
interval_series / interval_series2) on one GPU, against the unfused sequence of this library's own batched calls.

One process.  Every case is warmed up on both legs first; then ``--rounds`` rounds, each timing both legs once between two events
on torch's current stream, the legs alternating within a round; a record holds the median over the rounds per leg with min and max.
The legs:
  fused    one ``observe_negbinomial`` call, ``out=`` given: one launch;
  unfused  per pass ``compose_linear(D, 0, p)`` (the scaling substitution), ``mul_linear`` (pass 1) or ``mul`` by the power (from
           pass 2), the scaling by the row's entry (torch's broadcast multiply for f64, ``mul`` by a one-coefficient series for
           intervals), the addition (torch's) and ``derivative``; plus ``mul_linear`` for the next power: about five launches per
           pass.  It computes the same polynomial (the same bits only where no zero is added differently, and for intervals up to
           torch's unwidened addition); a record holds the largest difference between the legs over the largest coefficient.
A shape is ``BxL`` (rank 1) or ``BxN0xN1`` (rank 2, both variables run); ``--orders`` are cut to the ``L - 3`` the axis allows and
``degree_p1`` is ``L - order``, cut to the operation's own limit on ``3 * degree_p1 + order``.

    python tools/bench_series_observe_negbinomial.py --out profiles/r26/series_observe_negbinomial.json
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
    ap.add_argument("--orders", default="4,32", help="comma-separated orders K, each cut to L - 3 (default 4,32)")
    ap.add_argument("--rounds", type=int, default=7, help="rounds; the medians are over them (default 7)")
    ap.add_argument("--reps", type=int, default=100, help="fused calls per timing (default 100)")
    ap.add_argument("--reps-unfused", type=int, default=5, help="unfused sequences per timing (default 5)")
    ap.add_argument("--interval", action="store_true", help="the Interval<F64> twins (interval_series, interval_series2) instead of f64")
    ap.add_argument("--out", default=None, help="also write the records as a JSON list to this file (a file that exists is extended)")
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
    from genfer_amd import _series_call, interval_series, interval_series2, series, series2

    genfer_amd.init(0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(26)
    iv = args.interval
    lead = (2,) if iv else ()
    own = _series_call.NEGBIN_MAX[1 if iv else 0]
    results = []

    def rand(*shape, lo=0.5, width=1.0):
        v = lo + width * torch.rand(shape, dtype=torch.float64, generator=gen)
        return (torch.stack([v, v * (1.0 + 1e-9)]) if iv else v).to(dev)

    for shape in (args.shapes or (SHAPES_IV if iv else SHAPES)).split(","):
        dims = [int(t) for t in shape.lower().split("x")]
        B, item = dims[0], tuple(dims[1:])
        rank = len(item)
        mod = (interval_series if iv else series) if rank == 1 else (interval_series2 if iv else series2)
        rowmod = interval_series if iv else series
        a = rand(B, *item)
        x = rand(B, lo=0.1)
        p = rand(B, lo=0.2, width=0.6)
        c, zero = p * x, torch.zeros_like(p)  # (positive scalars: the bounds of p * x are the products of the bounds)
        for var in ((None,) if rank == 1 else (0, 1)):
            ax = -1 if var is None else var - 2
            L = item[ax]
            va = () if rank == 1 else (var,)
            for K in sorted({min(int(s), L - 3) for s in args.orders.split(",")}):
                if K < 0:
                    continue
                d = min(L - K, (own - K) // 3)
                ls = rowmod.lah_row(p, K)
                o = None if rank == 1 else min(item[1 + ax], d)
                rshape = (d,) if rank == 1 else ((d, o) if ax == -2 else (o, d))
                out = torch.empty(lead + (B,) + rshape, dtype=torch.float64, device=dev)
                # a series along the axis from per-item scalars: [.., B, len] at rank 1, with a unit axis beside it at rank 2
                along = (lambda t: t) if rank == 1 else ((lambda t: t[..., None]) if ax == -2 else (lambda t: t[..., None, :]))
                entry = ls[..., None] if rank == 1 else ls[..., None, None]  # [.., B, K + 1, 1(, 1)]: pass i is entry[..., i, :(, :)]
                plen = lambda n: n if rank == 1 else ((n, 1) if ax == -2 else (1, n))  # noqa: E731

                def fused():
                    mod.observe_negbinomial(a, *va, x, p, ls, d, out=out)

                def unfused():
                    D, total = a, None
                    P = along(torch.stack([c, p], dim=-1))
                    for i in range(K + 1):
                        Dn = D.narrow(ax, 0, d)
                        if rank == 2:
                            Dn = Dn.narrow(-3 - ax, 0, o)
                        S = mod.compose_linear(Dn, *va, zero, p)
                        nn = d if rank == 1 else tuple(S.shape[-2:])
                        U = S if i == 0 else (mod.mul_linear(S, *va, c, p, n=nn) if i == 1 else mod.mul(S, P, n=nn))
                        V = mod.mul(U, entry[:, :, i], n=nn) if iv else U * entry[:, i]
                        total = V if total is None else total + V
                        if i < K:
                            D = mod.derivative(D, *va, 1)
                            if i >= 1:
                                P = mod.mul_linear(P, *va, c, p, n=plen(min(d, P.shape[ax] + 1)))
                    return total

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
                rec = {"element": "interval" if iv else "f64", "B": B, "item": list(item), "order": K, "degree_p1": d}
                fused()
                rec["form"] = series.last_form()
                if var is not None:
                    rec["var"] = var
                for k, v in times.items():
                    rec.update({f"{k}_ms": round(med[k], 6), f"{k}_min_ms": round(min(v), 6), f"{k}_max_ms": round(max(v), 6)})
                launches = 2 * (K + 1) + 3 * K + max(K - 1, 0)  # S and V per pass; U, + and D from pass 1 on; P from pass 2 on
                rec.update({"unfused_over_fused": round(med["unfused"] / med["fused"], 3), "launches_unfused": launches, "legs_differ_rel": differ,
                            "rounds": args.rounds})
                results.append(rec)
                print(json.dumps(rec), flush=True)
    slower = [r for r in results if r["unfused_over_fused"] <= 1.0]
    summary = {"summary": True, "device": torch.cuda.get_device_properties(0).name, "cases": len(results),
               "min_unfused_over_fused": min((r["unfused_over_fused"] for r in results), default=None),
               "rows_where_fused_is_not_faster": [{k: r.get(k) for k in ("element", "B", "item", "var", "order", "unfused_over_fused")} for r in slower]}
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        before = json.load(open(args.out)) if os.path.exists(args.out) else []  # (the f64 run's records stay in front of --interval's)
        with open(args.out, "w") as fh:
            json.dump(before + results + [summary], fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
