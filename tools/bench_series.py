#!/usr/bin/env python3
"""Batched series (genfer_amd.series) against the per-row loop through the handle API, on one GPU.

For each operation and each (B, n) it times, between two events on torch's current stream after a warm-up,
  (a) the batched call, and
  (b) the per-row loop  from_torch(row) -> handle op -> to_torch(out[row])  on min(B, --loop-rows) rows, scaled to B
      (the only way to do this before the batched entry points existed),
and prints one JSON line per case: both times, their ratio, the algorithmic GB/s (8 * B * (nx + ny + n) bytes) and GMAC/s of
the batched call, and which form ran.  --form A|B asks for a form (dispatch thresholds are set from such sweeps).

--ops compose,pow: a shape is BxN or BxNxM with nf = ng = M (default M = N) for compose; pow raises to --pow-e.  compose has a
third leg, (c) the chain of nf - 1 series.mul calls each followed by an add into coefficient 0 on the same tensors (what a
caller could do before compose existed), reported as chain_ms and chain_over_batched.  Multiply-adds are counted at the compact
lengths the definition uses.

--interval: the same on interval tensors [2, B, n] (genfer_amd.interval_series against the IntervalTaylorPoly per-row loop), n
capped at 2048; bytes and multiply-adds count interval elements (16 bytes, one interval multiply-add).

--ops corr,backward (f64 only): `corr` times series.corr(g, y) at every shape against series.mul of the same (B, n) in the same
process and against the three-call emulation torch.flip -> series.mul -> torch.flip (corr_over_mul, flip_over_corr).  `backward`
times forward + backward of each of the six operations at --backward-shapes (compose with nf = min(n, 64)), and for compose the
transposed Horner kernel against gf formed by a Python chain of nf - 1 series.corr calls: alone (adj_ms, chain_ms) and inside the
same forward + backward (fb_chain_ms).

    python tools/bench_series.py > profiles/r07/series_batch.json
    python tools/bench_series.py --ops corr,backward --no-loop > profiles/r10/series_autograd.json
    python tools/bench_series.py --ops compose,pow --shapes 4096x16,4096x64,65536x32,1024x256,64x1024x64,1x4096x16
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
KNOWN_OPS = ("mul", "div", "exp", "log", "compose", "pow", "corr", "backward")
BACKWARD_SHAPES = "4096x64,65536x32,1024x256,64x1024"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ops", default=OPS, help=f"comma-separated operations out of {','.join(KNOWN_OPS)} (default {OPS})")
    ap.add_argument("--shapes", default=SHAPES, help=f"comma-separated BxN cases, BxNxM for compose with nf = ng = M (default {SHAPES})")
    ap.add_argument("--backward-shapes", default=BACKWARD_SHAPES, help=f"the BxN cases of --ops backward (default {BACKWARD_SHAPES})")
    ap.add_argument("--pow-e", type=int, default=5, help="the exponent of pow (default 5)")
    ap.add_argument("--form", choices=["auto", "A", "B"], default="auto", help="ask the library for a form (default: its thresholds)")
    ap.add_argument("--loop-rows", type=int, default=256, help="rows the per-row loop is timed on (scaled to B)")
    ap.add_argument("--budget-ms", type=float, default=300.0, help="time each leg repeats for, roughly")
    ap.add_argument("--no-loop", action="store_true", help="skip leg (b)")
    ap.add_argument("--interval", action="store_true", help="interval tensors [2, B, n]: interval_series against the IntervalTaylorPoly loop (n <= 2048)")
    args = ap.parse_args(argv)
    for op in args.ops.split(","):
        if op not in KNOWN_OPS:
            ap.error(f"unknown operation '{op}'")
        if op in ("corr", "backward") and args.interval:
            ap.error(f"'{op}' is f64 only")
    return args


def compose_macs(nf, ng, n):
    """multiply-adds of one item at the compact lengths of the Horner steps"""
    macs, lr = 0, 1
    for _ in range(nf - 1):
        L = min(lr + ng - 1, n)
        macs += sum(min(k + 1, lr) - max(0, k + 1 - ng) for k in range(L))
        lr = L
    return macs


def pow_macs(nx, e, n):
    macs, la, lb = 0, 1, nx
    prod = lambda a, b, L: sum(min(k + 1, a) - max(0, k + 1 - b) for k in range(L))  # noqa: E731
    while e > 0:
        if e & 1:
            L = min(la + lb - 1, n)
            macs += prod(la, lb, L)
            la = L
        e >>= 1
        if e > 0:
            L = min(2 * lb - 1, n)
            macs += prod(lb, lb, L)
            lb = L
    return macs


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


def chain_adj(series, torch, gh, g, nf):
    """compose_adj before it had a kernel: nf - 1 series.corr calls at the compact lengths, coefficient 0 of each collected"""
    n, ng = gh.shape[-1], g.shape[-1]
    ls = [min(1 + (nf - 1 - i) * (ng - 1), n) for i in range(nf)]
    a = gh[..., :ls[0]]
    out = torch.empty(gh.shape[:-1] + (nf,), dtype=torch.float64, device=gh.device)
    out[..., 0] = a[..., 0]
    for i in range(nf - 1):
        a = series.corr(a, g[..., :min(ng, a.shape[-1])], ls[i + 1])
        out[..., i + 1] = a[..., 0]
    return out


def bench_corr(torch, series, args, x, y, out, B, n):
    t_corr, reps = timed(torch, lambda: series.corr(x, y, out=out), args.budget_ms)
    form = series.last_form()
    t_mul, _ = timed(torch, lambda: series.mul(x, y, out=out), args.budget_ms)
    form_mul = series.last_form()
    t_flip, _ = timed(torch, lambda: torch.flip(series.mul(torch.flip(x, [-1]), y), [-1]), args.budget_ms)
    return {"op": "corr", "B": B, "n": n, "form": form, "mul_form": form_mul, "corr_ms": round(t_corr, 6), "corr_reps": reps,
            "mul_ms": round(t_mul, 6), "flip_mul_flip_ms": round(t_flip, 6), "corr_over_mul": round(t_corr / t_mul, 3),
            "flip_over_corr": round(t_flip / t_corr, 3), "GMACps": round(B * n * (n + 1) / 2.0 / (t_corr * 1e-3) / 1e9, 3)}


def bench_backward(torch, series, args, B, n, gen, dev):
    """forward + backward of each operation, one record a line"""
    import math

    x = (0.5 + torch.rand((B, n), dtype=torch.float64, generator=gen) / n).to(dev).requires_grad_()
    y = (0.5 + torch.rand((B, n), dtype=torch.float64, generator=gen) / n).to(dev)
    y[:, 0] += 2.0
    y.requires_grad_()
    gz = torch.rand((B, n), dtype=torch.float64, generator=gen).to(dev)
    nf = min(n, 64)
    seeds = {f: torch.tensor([getattr(math, f)(v) for v in x.detach()[:, 0].tolist()], dtype=torch.float64).to(dev) for f in ("exp", "log")}
    calls = {"mul": lambda: series.mul(x, y), "div": lambda: series.div(x, y), "exp": lambda: series.exp(x, seed=seeds["exp"]),
             "log": lambda: series.log(x, seed=seeds["log"]), "pow": lambda: series.pow(x, args.pow_e),
             "compose": lambda: series.compose(x[:, :nf], y)}
    recs = []
    for op, call in calls.items():
        def fb():
            x.grad = y.grad = None
            call().backward(gz)

        def fwd():
            with torch.no_grad():
                call()

        t_fb, reps = timed(torch, fb, args.budget_ms)
        t_f, _ = timed(torch, fwd, args.budget_ms)
        rec = {"op": "backward", "of": op, "B": B, "n": n, "forward_backward_ms": round(t_fb, 6), "reps": reps, "forward_ms": round(t_f, 6),
               "backward_over_forward": round((t_fb - t_f) / t_f, 3)}
        if op == "compose":
            gd, yd = gz, y.detach()
            t_adj, _ = timed(torch, lambda: series._compose_adj(gd, yd, nf), args.budget_ms)
            t_chain, _ = timed(torch, lambda: chain_adj(series, torch, gd, yd, nf), args.budget_ms)
            kernel = series._compose_adj
            series._compose_adj = lambda gh, g, k: chain_adj(series, torch, gh, g, k)
            try:
                t_fbc, _ = timed(torch, fb, args.budget_ms)
            finally:
                series._compose_adj = kernel
            rec.update({"nf": nf, "adj_ms": round(t_adj, 6), "chain_ms": round(t_chain, 6), "chain_over_adj": round(t_chain / t_adj, 3),
                        "fb_chain_ms": round(t_fbc, 6), "fb_chain_over_fb": round(t_fbc / t_fb, 3)})
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    return recs


def main(argv=None):
    args = parse_args(argv)
    import torch

    import genfer_amd
    from genfer_amd import series

    genfer_amd.init(0)
    iv = args.interval
    if iv:
        from genfer_amd import interval_series as series  # noqa: F811  (the same six functions on [2, B, n])
    TP = genfer_amd.IntervalTaylorPoly if iv else genfer_amd.TaylorPoly
    W = 2 if iv else 1
    item = (lambda t, b: t[:, b]) if iv else (lambda t, b: t[b])  # row b of a batch, with its planes
    dev = torch.device("cuda", 0)
    series.set_form(None if args.form == "auto" else args.form)
    gen = torch.Generator(device="cpu").manual_seed(7)
    results = []
    for shape in args.shapes.split(","):
        dims = [int(t) for t in shape.lower().split("x")]
        B, n = dims[0], dims[1]
        if iv:
            n = min(n, 2048)
        m = min(dims[2], n) if len(dims) > 2 else n  # nf = ng of compose
        # bounded results at every order: a dominant constant term in the divisor, a small argument for exp
        x = (0.5 + torch.rand((B, n), dtype=torch.float64, generator=gen) / n).to(dev)
        y = (0.5 + torch.rand((B, n), dtype=torch.float64, generator=gen) / n).to(dev)
        y[:, 0] += 2.0
        if iv:  # [2, B, n]: lower bounds as above, about 2^-30 relative width
            x = torch.stack([x, x * (1.0 + 2.0**-30)])
            y = torch.stack([y, y * (1.0 + 2.0**-30)])
        out = torch.empty((B, n) if not iv else (2, B, n), dtype=torch.float64, device=dev)
        for op in args.ops.split(","):
            if op == "backward":  # its own shapes, below
                continue
            if op == "corr":
                results.append(bench_corr(torch, series, args, x, y, out, B, n))
                print(json.dumps(results[-1]), flush=True)
                continue
            seed = None
            if op in ("exp", "log"):
                seed = torch.tensor([getattr(math, op)(v) for v in x[..., 0].reshape(-1).cpu().tolist()], dtype=torch.float64)
                seed = seed.reshape(x.shape[:-1]).to(dev)  # (intervals: the bounds' own exp / log, unwidened -- timing only)

            fc, gc = x[..., :m], y[..., :m]  # compose: f and g as views of the same tensors
            step = torch.empty_like(out)

            def batched():
                if op in ("mul", "div"):
                    getattr(series, op)(x, y, out=out)
                elif op == "compose":
                    series.compose(fc, gc, n=n, out=out)
                elif op == "pow":
                    series.pow(x, args.pow_e, out=out)
                else:
                    getattr(series, op)(x, seed=seed, out=out)

            t_batch, reps_a = timed(torch, batched, args.budget_ms)
            form = series.last_form()
            rows = min(B, args.loop_rows)

            def loop():
                for b in range(rows):
                    p = TP.from_torch(item(x, b))
                    if op == "mul":
                        r = p * TP.from_torch(item(y, b))
                    elif op == "div":
                        r = p / TP.from_torch(item(y, b))
                    elif op == "compose":
                        r = TP.from_torch(item(fc, b), degrees_p1=(n,)).subst_var(0, TP.from_torch(item(gc, b), degrees_p1=(n,)))
                        item(out, b).zero_()
                        r.to_torch(out=item(out, b)[..., :r.coeffs_shape()[0]])
                        continue
                    elif op == "pow":
                        r = p.pow(args.pow_e)
                    else:
                        r = p.exp() if op == "exp" else p.log()
                    r.to_torch(out=item(out, b))

            def chain():  # compose before compose: nf - 1 products at full length, each followed by an add into coefficient 0
                a, b = step, out
                if (m - 1) % 2 == 0:
                    a, b = b, a  # the last product lands in `out`
                a.zero_()
                a[..., 0] = fc[..., m - 1]
                for i in range(m - 2, -1, -1):
                    series.mul(a, gc, n=n, out=b)
                    b[..., 0] += fc[..., i]  # (intervals: unwidened, the cost of the add is what is timed)
                    a, b = b, a

            rec = {"op": op, "B": B, "n": n, "form": form, **({"interval": True} if iv else {}), "batched_ms": round(t_batch, 6), "batched_reps": reps_a}
            macs = B * n * (n + 1) / 2.0
            nbytes = 8.0 * W * B * (n + (n if op in ("mul", "div") else 0) + n)
            if op == "compose":
                rec["nf"] = rec["ng"] = m
                macs, nbytes = float(B * compose_macs(m, m, n)), 8.0 * W * B * (2 * m + n)
            elif op == "pow":
                rec["e"] = args.pow_e
                macs = float(B * pow_macs(n, args.pow_e, n))
            rec["algorithmic_GBps"] = round(nbytes / (t_batch * 1e-3) / 1e9, 3)
            rec["GMACps"] = round(macs / (t_batch * 1e-3) / 1e9, 3)
            if not args.no_loop:
                t_loop, reps_b = timed(torch, loop, args.budget_ms)
                t_loop *= B / rows
                rec.update({"loop_ms": round(t_loop, 6), "loop_rows": rows, "loop_reps": reps_b, "loop_over_batched": round(t_loop / t_batch, 3)})
            if op == "compose" and m > 1:
                t_chain, reps_c = timed(torch, chain, args.budget_ms)
                rec.update({"chain_ms": round(t_chain, 6), "chain_reps": reps_c, "chain_over_batched": round(t_chain / t_batch, 3)})
            results.append(rec)
            print(json.dumps(rec), flush=True)
    if "backward" in args.ops.split(","):
        for shape in args.backward_shapes.split(","):
            B, n = (int(t) for t in shape.lower().split("x"))
            results += bench_backward(torch, series, args, B, n, gen, dev)
    series.set_form(None)
    props = torch.cuda.get_device_properties(0)
    corr_recs = [r for r in results if r["op"] == "corr"]
    adj_recs = [r for r in results if "chain_over_adj" in r]
    if corr_recs or adj_recs:  # the three comparisons of DESIGN 3.15: met (true) or missed (false), None where not run
        print(json.dumps({"summary": "autograd",
                          "max_corr_over_mul": max([r["corr_over_mul"] for r in corr_recs], default=None),
                          "corr_no_slower_than_1.1x_mul": all(r["corr_over_mul"] <= 1.1 for r in corr_recs) if corr_recs else None,
                          "min_flip_over_corr": min([r["flip_over_corr"] for r in corr_recs], default=None),
                          "corr_faster_than_flip_mul_flip": all(r["flip_over_corr"] > 1.0 for r in corr_recs) if corr_recs else None,
                          "min_chain_over_adj": min([r["chain_over_adj"] for r in adj_recs], default=None),
                          "compose_adj_no_slower_than_chain": all(r["chain_over_adj"] >= 1.0 for r in adj_recs) if adj_recs else None}))
    print(json.dumps({"summary": True, "device": props.name, "asked_form": args.form, "interval": iv, "cases": len(results),
                      "min_ratio_B_ge_256": min([r["loop_over_batched"] for r in results if r["B"] >= 256 and "loop_over_batched" in r], default=None),
                      "min_ratio_B_lt_256": min([r["loop_over_batched"] for r in results if r["B"] < 256 and "loop_over_batched" in r], default=None),
                      "min_chain_over_batched": min([r["chain_over_batched"] for r in results if "chain_over_batched" in r], default=None)}))


if __name__ == "__main__":
    main()
