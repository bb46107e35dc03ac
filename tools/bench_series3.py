#!/usr/bin/env python3
"""Batched trivariate series (genfer_amd.series3) against the per-item loop through the handle API, on one GPU.

For each operation and each (B, n0, n1, n2) it times, between two events on torch's current stream after a warm-up,
  (a) the batched call, and
  (b) the per-item loop  from_torch(item) -> handle op -> to_torch(out[item])  on min(B, --loop-items) items, scaled to B
      (the only way to do this before the batched entry points existed),
and prints one JSON line per case: both times, their ratio, and the GMAC/s of the batched call (multiply-adds of the row
products, counted over the stored coefficients).  A summary line states the two standing targets of batched calls against the
loop measured in the same run: at least 10x for B >= 256, no slower than 1.1x for B < 256; every row says whether it met its own.

``--ops compose,pow`` times ``series3.compose(f, g, var)`` for var = 0, 1, 2 (f and g of the full shape) and ``series3.pow(x, 5)``
against the handle loop (``subst_var`` / ``pow``) and, for compose, also against
  (c) the Python chain of ``series3.mul`` calls with a slice add after each -- the other route a caller had before.

``--interval``: the same on ``Interval<F64>`` tensors ``[2, B, n0, n1, n2]`` (genfer_amd.interval_series3) against the loop over
``IntervalTaylorPoly`` handles, every shape with ``n0 * n1 * n2`` capped at 2048 (the longest axis is halved until the item fits), over
mul, div, exp, log, compose (var 0, 1, 2) and pow e = 5 by default; the chain of leg (c) is ``interval_series3.mul`` plus the slice add (a plain ``+=`` on both
planes, not an outward-rounded interval add: a timing leg only).

    python tools/bench_series3.py > profiles/r17/series3.json
    python tools/bench_series3.py --interval > profiles/r21/series3_interval.json
    python tools/bench_series3.py --ops compose,pow > profiles/r20/series3_compose.json
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
MORE_OPS = "compose,pow"  # on request: three rows per shape for compose (one per variable), one for pow
POW_E = 5


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ops", default=None, help=f"comma-separated operations out of {OPS},{MORE_OPS} (default: {OPS}; with --interval all six)")
    ap.add_argument("--interval", action="store_true",
                    help="Interval<F64> tensors [2, B, n0, n1, n2] (interval_series3), n0 * n1 * n2 capped at 2048")
    ap.add_argument("--shapes", default=SHAPES, help=f"comma-separated BxN0xN1xN2 cases (default {SHAPES})")
    ap.add_argument("--loop-items", type=int, default=256, help="items the per-item loop is timed on (scaled to B)")
    ap.add_argument("--budget-ms", type=float, default=300.0, help="time each leg repeats for, roughly")
    ap.add_argument("--no-loop", action="store_true", help="skip leg (b)")
    args = ap.parse_args(argv)
    if args.ops is None:
        args.ops = OPS + "," + MORE_OPS if args.interval else OPS
    for op in args.ops.split(","):
        if op not in (OPS + "," + MORE_OPS).split(","):
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


def product_macs(a, b, L):
    """multiply-adds of the product of two items of the stored shapes a and b truncated at L"""
    return math.prod(sum(min(k + 1, a[i]) - max(0, k + 1 - b[i]) for k in range(L[i])) for i in range(3))


def compose_steps(n, var):
    """(stored shape of res, compact shape of the product) for every step of compose with f and g of the full shape n"""
    r = tuple(1 if a == var else n[a] for a in range(3))
    for _ in range(n[var] - 1):
        L = tuple(min(r[a] + n[a] - 1, n[a]) for a in range(3))
        yield r, L
        r = L


def pow_macs(n, e):
    res, base, total = (1, 1, 1), tuple(n), 0.0
    compact = lambda a, b: tuple(min(a[i] + b[i] - 1, n[i]) for i in range(3))  # noqa: E731
    while e > 0:
        if e & 1:
            total += product_macs(res, base, compact(res, base))
            res = compact(res, base)
        e >>= 1
        if e > 0:
            total += product_macs(base, base, compact(base, base))
            base = compact(base, base)
    return total


def target(B, ratio):
    """the standing targets of a batched call against the loop, for one row"""
    return "met" if ratio >= (10.0 if B >= 256 else 1 / 1.1) else "missed"


def cap_item(n, most):
    """halve the longest axis until n0 * n1 * n2 <= most"""
    n = list(n)
    while math.prod(n) > most:
        a = n.index(max(n))
        n[a] = (n[a] + 1) // 2
    return tuple(n)


def bench_compose_pow(args, torch, series3, TP, op, B, n, f, g, out, results, item, tag):
    """compose: one row per variable; pow: one row at e = POW_E.  The series axes are addressed from the right: an interval tensor has
    the plane axis in front of the batch"""
    for var in (0, 1, 2) if op == "compose" else (None,):
        if op == "compose":
            work = sum(product_macs(r, n, L) for r, L in compose_steps(n, var))

            def batched():
                series3.compose(f, g, var=var, out=out)

            def chain():
                res = 0.0 + f.narrow(var - 3, n[var] - 1, 1)
                head = (Ellipsis,) + tuple(slice(0, 1) if a == var else slice(None) for a in range(3))
                for i in range(n[var] - 2, -1, -1):
                    res = series3.mul(res, g, n=tuple(min(res.shape[a - 3] + n[a] - 1, n[a]) for a in range(3)))
                    res[head] += f.narrow(var - 3, i, 1)
                out.zero_()
                out[..., :res.shape[-3], :res.shape[-2], :res.shape[-1]] = res
        else:
            work = pow_macs(n, POW_E)

            def batched():
                series3.pow(f, POW_E, out=out)

        t_batch, reps_a = timed(torch, batched, args.budget_ms)
        items = min(B, args.loop_items)

        def loop():
            for b in range(items):
                p = TP.from_torch(item(f, b))
                r = p.subst_var(var, TP.from_torch(item(g, b))) if op == "compose" else p.pow(POW_E)
                r.to_torch(out=item(out, b))

        rec = {**tag, "op": op, "B": B, "n0": n[0], "n1": n[1], "n2": n[2], "batched_ms": round(t_batch, 6), "batched_reps": reps_a,
               "GMACps": round(B * work / (t_batch * 1e-3) / 1e9, 3)}
        rec.update({"var": var} if op == "compose" else {"e": POW_E})
        if not args.no_loop:
            t_loop, reps_b = timed(torch, loop, args.budget_ms)
            t_loop *= B / items
            ratio = t_loop / t_batch
            rec.update({"loop_ms": round(t_loop, 6), "loop_items": items, "loop_reps": reps_b, "loop_over_batched": round(ratio, 3),
                        "target": target(B, ratio)})
            if op == "compose":
                t_chain, reps_c = timed(torch, chain, args.budget_ms)
                rec.update({"chain_ms": round(t_chain, 6), "chain_reps": reps_c, "chain_over_batched": round(t_chain / t_batch, 3)})
        results.append(rec)
        print(json.dumps(rec), flush=True)


def main(argv=None):
    args = parse_args(argv)
    import torch

    import genfer_amd
    from genfer_amd import interval_series3, series3

    genfer_amd.init(0)
    iv = args.interval
    TP = genfer_amd.IntervalTaylorPoly if iv else genfer_amd.TaylorPoly
    if iv:
        series3 = interval_series3
    item = (lambda t, b: t[:, b]) if iv else (lambda t, b: t[b])
    tag = {"element": "interval"} if iv else {}
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(7)
    results = []
    for shape in args.shapes.split(","):
        B, *n = (int(t) for t in shape.lower().split("x"))
        if iv:
            n = list(cap_item(n, interval_series3.MAX_ELEMS))
        N = math.prod(n)
        # bounded results at every order: a dominant constant term in the divisor, a small argument for exp
        x = (0.5 + torch.rand((B, *n), dtype=torch.float64, generator=gen) / N).to(dev)
        y = (0.5 + torch.rand((B, *n), dtype=torch.float64, generator=gen) / N).to(dev)
        y[:, 0, 0, 0] += 2.0
        if iv:  # (lo, hi) planes about 2^-20 apart; the loop indexes items behind the plane axis
            x = torch.stack([x, x * (1.0 + 2.0**-20)])
            y = torch.stack([y, y * (1.0 + 2.0**-20)])
        out = torch.empty(((2,) if iv else ()) + (B, *n), dtype=torch.float64, device=dev)
        for op in args.ops.split(","):
            if op in MORE_OPS.split(","):
                bench_compose_pow(args, torch, series3, TP, op, B, tuple(n), x, y if op == "compose" else None, out, results, item, tag)
                continue
            seed = None
            if op in ("exp", "log") and iv:  # a host's seeds: libm, one ulp outwards
                s = torch.tensor([[getattr(math, op)(v) for v in pl] for pl in x[:, :, 0, 0, 0].cpu().tolist()], dtype=torch.float64)
                seed = torch.stack([torch.nextafter(s[0], s[0] - 1.0), torch.nextafter(s[1], s[1] + 1.0)]).to(dev)
            elif op in ("exp", "log"):
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
                    p = TP.from_torch(item(x, b))
                    if op == "mul":
                        r = p * TP.from_torch(item(y, b))
                    elif op == "div":
                        r = p / TP.from_torch(item(y, b))
                    else:
                        r = p.exp() if op == "exp" else p.log()
                    r.to_torch(out=item(out, b))

            rec = {**tag, "op": op, "B": B, "n0": n[0], "n1": n[1], "n2": n[2], "batched_ms": round(t_batch, 6), "batched_reps": reps_a,
                   "GMACps": round(B * macs(n) / (t_batch * 1e-3) / 1e9, 3)}
            if not args.no_loop:
                t_loop, reps_b = timed(torch, loop, args.budget_ms)
                t_loop *= B / items
                rec.update({"loop_ms": round(t_loop, 6), "loop_items": items, "loop_reps": reps_b, "loop_over_batched": round(t_loop / t_batch, 3),
                            "target": target(B, t_loop / t_batch)})
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
