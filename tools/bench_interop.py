#!/usr/bin/env python3
"""Device interop rates: TaylorPoly.from_torch (import) and to_torch (export) of float64 tensors on the MI355X.

Cases: f64 and interval, n^3 for n = 64, 128, 256, and three source / destination layouts — contiguous, a last-axis slice
(import: t[..., ::2] of a twice-as-wide tensor; export: [..., :n] of a wider buffer) and permute(2, 1, 0).  Each time is the
mean over `--reps` calls between two hipEvents on torch's current stream (the calls join that stream both ways, so the events
bracket the copies).  TB/s = (bytes read + bytes written) / time, logical bytes: 2 * 8 * elements (planes included).
Next to each contiguous case: the host round trip of the same tensor, t.cpu().numpy() -> new() -> array() ->
torch.from_numpy(...).cuda(), against from_torch + to_torch, both timed on the host clock to a synchronise.
Prints one JSON line; --out FILE also writes it there."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import genfer_amd

    genfer_amd.init(0)
    dev = torch.device("cuda", 0)
    classes = {"f64": genfer_amd.TaylorPoly, "interval": genfer_amd.IntervalTaylorPoly}

    def timed(fn, reps):
        fn()  # warm: pool blocks, code objects
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps * 1e-3  # seconds per call

    def host_timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    results = []
    for kind, TP in classes.items():
        lead = (2,) if kind == "interval" else ()
        for n in (int(s) for s in args.sizes.split(",")):
            shape = lead + (n, n, n)
            elems = 2 * n**3 if lead else n**3
            moved = 2 * 8 * elems
            base = torch.rand(shape, dtype=torch.float64, device=dev)
            perm = (0, 3, 2, 1) if lead else (2, 1, 0)
            sources = {
                "contiguous": base,
                "last_axis_slice": torch.rand(shape[:-1] + (2 * n,), dtype=torch.float64, device=dev)[..., ::2],
                "permute_2_1_0": torch.rand(shape, dtype=torch.float64, device=dev).permute(*perm),
            }
            wide = torch.empty(shape[:-1] + (n + 8,), dtype=torch.float64, device=dev)
            dests = {
                "contiguous": torch.empty(shape, dtype=torch.float64, device=dev),
                "last_axis_slice": wide[..., :n],
                "permute_2_1_0": torch.empty(shape, dtype=torch.float64, device=dev).permute(*perm),
            }
            handle = TP.from_torch(base)
            reps = args.reps if n <= 128 else max(5, args.reps // 2)
            for layout in sources:
                src, dst = sources[layout], dests[layout]
                t_imp = timed(lambda: TP.from_torch(src), reps)
                t_exp = timed(lambda: handle.to_torch(out=dst), reps)
                assert torch.equal(TP.from_torch(src).to_torch(), src.contiguous()), (kind, n, layout)
                r = {"kind": kind, "n": n, "layout": layout, "bytes": moved,
                     "import_us": round(t_imp * 1e6, 2), "import_TBps": round(moved / t_imp / 1e12, 3),
                     "export_us": round(t_exp * 1e6, 2), "export_TBps": round(moved / t_exp / 1e12, 3)}
                if layout == "contiguous":
                    deg = shape[1:] if lead else shape
                    hreps = max(2, reps // 5)
                    t_host = host_timed(lambda: torch.from_numpy(TP.new(src.cpu().numpy(), deg).array()).to(dev), hreps)
                    t_dev = host_timed(lambda: TP.from_torch(src).to_torch(), hreps)
                    r.update({"host_round_trip_ms": round(t_host * 1e3, 3), "device_round_trip_ms": round(t_dev * 1e3, 3),
                              "round_trip_speedup": round(t_host / t_dev, 1)})
                results.append(r)
            del handle, sources, dests, wide, base
            torch.cuda.empty_cache()

    def pick(kind, n, layout):
        for r in results:
            if (r["kind"], r["n"], r["layout"]) == (kind, n, layout):
                return r
        return None

    summary = {}
    for key, (kind, n, layout) in {"f64_256_contiguous": ("f64", 256, "contiguous"), "f64_256_permute": ("f64", 256, "permute_2_1_0"),
                                   "f64_128_contiguous": ("f64", 128, "contiguous")}.items():
        r = pick(kind, n, layout)
        if r:
            summary[key] = {k: r[k] for k in r if k.endswith("TBps") or k.endswith("speedup")}
    line = json.dumps({"metric": "TaylorPoly device interop", "unit": "TB/s (read + write)", "device": torch.cuda.get_device_name(0),
                       "reps": args.reps, "summary": summary, "cases": results})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
