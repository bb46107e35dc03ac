#!/usr/bin/env python3
"""Batched bivariate series (genfer_amd.series2) against the per-item loop through the handle API, on one GPU.

For each operation and each (B, n0, n1) it times, between two events on torch's current stream after a warm-up,
  (a) the batched call, and
  (b) the per-item loop  from_torch(item) -> handle op -> to_torch(out[item])  on min(B, --loop-items) items, scaled to B
      (the only way to do this before the batched entry points existed),
and prints one JSON line per case: both times, their ratio, and the GMAC/s of the batched call (multiply-adds of the row
products, counted over the stored coefficients).  A summary line states the two standing targets of batched calls against the
loop measured in the same run: at least 10x for B >= 256, no slower than 1.1x for B < 256.

``--ops compose,pow`` (not in the default set): compose runs once per substituted variable (``var`` in the record) against
``subst_var`` in the loop, and also against (c) the Python chain of ``series2.mul`` calls with the slice added after each -- the
way to compose before the fused kernel -- with its own target, no slower than 1.1x that chain; pow runs at ``--pow-e``.

``--interval``: the same on ``Interval<F64>`` tensors ``[2, B, n0, n1]`` (genfer_amd.interval_series2) against the loop over
``IntervalTaylorPoly`` handles, every shape with ``n0 * n1`` capped at 2048 (the longer axis is halved until the item fits); the
chain of leg (c) is ``interval_series2.mul`` plus the slice add (exact where the running result's slice is still [0,0], one
``torch`` add per bound otherwise: a caller's chain, not the definition).

    python tools/bench_series2.py > profiles/r11/series2.json
    python tools/bench_series2.py --ops compose,pow --budget-ms 150 > profiles/r12/series2_compose.json
    python tools/bench_series2.py --interval --ops mul,div,exp,log,compose,pow --budget-ms 100 > profiles/r13/series2_interval.json
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = "4096x8x8,65536x4x8,1024x16x16,256x64x64,64x32x128,1x64x64"
OPS = "mul,div,exp,log"
KNOWN_OPS = OPS + ",compose,pow"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ops", default=OPS, help=f"comma-separated operations out of {KNOWN_OPS} (default: {OPS})")
    ap.add_argument("--shapes", default=SHAPES, help=f"comma-separated BxN0xN1 cases (default {SHAPES})")
    ap.add_argument("--loop-items", type=int, default=256, help="items the per-item loop is timed on (scaled to B)")
    ap.add_argument("--budget-ms", type=float, default=300.0, help="time each leg repeats for, roughly")
    ap.add_argument("--no-loop", action="store_true", help="skip leg (b)")
    ap.add_argument("--pow-e", type=int, default=5, help="the exponent of pow (default 5)")
    ap.add_argument("--interval", action="store_true", help="Interval<F64> tensors [2, B, n0, n1] (interval_series2), n0 * n1 capped at 2048")
    args = ap.parse_args(argv)
    for op in args.ops.split(","):
        if op not in KNOWN_OPS.split(","):
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


def macs(n0, n1):
    """multiply-adds of the dense row products of one item: sum over (k0, j0 <= k0) of a row product of n1 (n1 + 1) / 2"""
    return n0 * (n0 + 1) / 2.0 * n1 * (n1 + 1) / 2.0


def compose_macs(n0, n1, var):
    """multiply-adds of compose's dense steps: step s multiplies a result of compact shape min(1 + s (n - 1), n) on the
    substituted axis by a dense g, truncated at the next compact shape; counted over the stored coefficients"""
    slices = (n0, n1)[var]
    total, r = 0.0, [1, 1]
    r[1 - var] = (n0, n1)[1 - var]
    for _ in range(slices - 1):
        L = [min(r[0] + n0 - 1, n0), min(r[1] + n1 - 1, n1)]
        per_axis = [sum(min(k + 1, r[a]) - max(0, k + 1 - (n0, n1)[a]) for k in range(L[a])) for a in (0, 1)]
        total += per_axis[0] * per_axis[1]
        r = L
    return total


def chain_compose(torch, series2, f, g, var, n):
    """compose as a caller writes it without the fused kernel: one series2.mul per slice and an add into the slice's place (with a
    leading plane axis for interval_series2: the ellipsis takes it)"""
    n0, n1 = n
    if var == 0:
        res = 0.0 + f[..., -1:, :]
        for i in range(f.shape[-2] - 2, -1, -1):
            res = series2.mul(res, g, n=(min(res.shape[-2] + g.shape[-2] - 1, n0), min(res.shape[-1] + g.shape[-1] - 1, n1)))
            res[..., 0, :f.shape[-1]] += f[..., i, :]
    else:
        res = 0.0 + f[..., :, -1:]
        for i in range(f.shape[-1] - 2, -1, -1):
            res = series2.mul(res, g, n=(min(res.shape[-2] + g.shape[-2] - 1, n0), min(res.shape[-1] + g.shape[-1] - 1, n1)))
            res[..., :f.shape[-2], 0] += f[..., :, i]
    return res


def cap_item(n0, n1, most):
    """halve the longer axis until n0 * n1 <= most"""
    while n0 * n1 > most:
        if n0 >= n1:
            n0 = (n0 + 1) // 2
        else:
            n1 = (n1 + 1) // 2
    return n0, n1


def main(argv=None):
    args = parse_args(argv)
    import torch

    import genfer_amd
    from genfer_amd import interval_series2, series2

    genfer_amd.init(0)
    iv = args.interval
    TP = genfer_amd.IntervalTaylorPoly if iv else genfer_amd.TaylorPoly
    if iv:
        series2 = interval_series2
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(7)
    results = []
    for shape in args.shapes.split(","):
        B, n0, n1 = (int(t) for t in shape.lower().split("x"))
        if iv:
            n0, n1 = cap_item(n0, n1, interval_series2.MAX_ELEMS)
        # bounded results at every order: a dominant constant term in the divisor, a small argument for exp
        x = (0.5 + torch.rand((B, n0, n1), dtype=torch.float64, generator=gen) / (n0 * n1)).to(dev)
        y = (0.5 + torch.rand((B, n0, n1), dtype=torch.float64, generator=gen) / (n0 * n1)).to(dev)
        y[:, 0, 0] += 2.0
        if iv:  # (lo, hi) planes about 2^-20 apart; the loop indexes items behind the plane axis
            x = torch.stack([x, x * (1.0 + 2.0**-20)])
            y = torch.stack([y, y * (1.0 + 2.0**-20)])
        item = (lambda t, b: t[:, b]) if iv else (lambda t, b: t[b])
        out = torch.empty(((2,) if iv else ()) + (B, n0, n1), dtype=torch.float64, device=dev)
        for op, var in [(o, v) for o in args.ops.split(",") for v in ((0, 1) if o == "compose" else (None,))]:
            seed = None
            if op in ("exp", "log"):
                if iv:  # a host's seeds: libm, one ulp outwards
                    s = torch.tensor([[getattr(math, op)(v) for v in pl] for pl in x[:, :, 0, 0].cpu().tolist()], dtype=torch.float64)
                    seed = torch.stack([torch.nextafter(s[0], s[0] - 1.0), torch.nextafter(s[1], s[1] + 1.0)]).to(dev)
                else:
                    seed = torch.tensor([getattr(math, op)(v) for v in x[:, 0, 0].cpu().tolist()], dtype=torch.float64).to(dev)

            def batched():
                if op in ("mul", "div"):
                    getattr(series2, op)(x, y, out=out)
                elif op == "compose":
                    series2.compose(x, y, var, out=out)
                elif op == "pow":
                    series2.pow(x, args.pow_e, out=out)
                else:
                    getattr(series2, op)(x, seed=seed, out=out)

            t_batch, reps_a = timed(torch, batched, args.budget_ms)
            items = min(B, args.loop_items)

            def loop():
                for b in range(items):
                    p = TP.from_torch(item(x, b))
                    if op == "mul":
                        r = p * TP.from_torch(item(y, b))
                    elif op == "div":
                        r = p / TP.from_torch(item(y, b))
                    elif op == "compose":
                        r = p.subst_var(var, TP.from_torch(item(y, b)))
                    elif op == "pow":
                        r = p.pow(args.pow_e)
                    else:
                        r = p.exp() if op == "exp" else p.log()
                    r.to_torch(out=item(out, b))

            work = macs(n0, n1)
            if op == "compose":
                work = compose_macs(n0, n1, var)
            elif op == "pow":  # the dense products of square-and-multiply, each at the full shape at most
                work *= bin(args.pow_e).count("1") + max(args.pow_e.bit_length() - 1, 0)
            rec = {**({"element": "interval"} if iv else {}), "op": op, "B": B, "n0": n0, "n1": n1, "batched_ms": round(t_batch, 6), "batched_reps": reps_a,
                   "GMACps": round(B * work / (t_batch * 1e-3) / 1e9, 3)}
            if op == "compose":
                rec["var"] = var
                t_chain, reps_c = timed(torch, lambda: chain_compose(torch, series2, x, y, var, (n0, n1)), args.budget_ms)
                rec.update({"chain_ms": round(t_chain, 6), "chain_reps": reps_c, "chain_over_batched": round(t_chain / t_batch, 3)})
            elif op == "pow":
                rec["e"] = args.pow_e
            if not args.no_loop:
                t_loop, reps_b = timed(torch, loop, args.budget_ms)
                t_loop *= B / items
                rec.update({"loop_ms": round(t_loop, 6), "loop_items": items, "loop_reps": reps_b, "loop_over_batched": round(t_loop / t_batch, 3)})
            results.append(rec)
            print(json.dumps(rec), flush=True)
    props = torch.cuda.get_device_properties(0)
    big = [r["loop_over_batched"] for r in results if r["B"] >= 256 and "loop_over_batched" in r]
    small = [r["loop_over_batched"] for r in results if r["B"] < 256 and "loop_over_batched" in r]
    chain = [r["chain_over_batched"] for r in results if "chain_over_batched" in r]
    print(json.dumps({"summary": True, "device": props.name, "cases": len(results),
                      "min_ratio_B_ge_256": min(big, default=None), "target_10x_met_B_ge_256": all(v >= 10.0 for v in big) if big else None,
                      "min_ratio_B_lt_256": min(small, default=None), "target_no_slower_than_1.1x_met_B_lt_256": all(v >= 1 / 1.1 for v in small) if small else None,
                      "min_ratio_chain": min(chain, default=None), "target_no_slower_than_1.1x_chain_met": all(v >= 1 / 1.1 for v in chain) if chain else None}))


if __name__ == "__main__":
    main()
