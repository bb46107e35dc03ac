"""Wave-slot occupancy of the tiled product's launches from rocprofv3 counter passes (counters-only runs, one CSV per pass):

    rocprofv3 --pmc SQ_BUSY_CYCLES SQ_WAVE_CYCLES --output-format csv -d A -o pmc -- python3 bench.py --steps 3 --warmup 1
    rocprofv3 --pmc SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE --output-format csv -d B -o pmc -- python3 bench.py --steps 3 --warmup 1
    python3 tools/pmc_occupancy.py out.json A/.../pmc_counter_collection.csv B/.../pmc_counter_collection.csv

Per kernel (k_conv_tiled instantiations and k_conv_reduce), mean per launch.  Units as read in DESIGN 3.1: GRBM_GUI_ACTIVE
sums the 8 XCDs; SQ_WAVE_CYCLES and SQ_ACTIVE_INST_* count once per four clocks; SQ_BUSY_CYCLES sums 32 shader engines.
    occupied  = 4 SQ_WAVE_CYCLES / (4096 wave slots x clocks)       share of the launch in which a wave slot holds a wave
    se_busy   = SQ_BUSY_CYCLES / 32 / clocks
    valu_busy = 4 SQ_ACTIVE_INST_VALU / (1024 SIMDs x clocks)
"""
import csv
import json
import re
import sys

out, files = sys.argv[1], sys.argv[2:]
per = {}
for f in files:
    for r in csv.DictReader(open(f)):
        m = re.search(r"(k_conv_tiled<[^>]*>|k_conv_reduce)", r["Kernel_Name"])
        if not m:
            continue
        d = per.setdefault(m.group(1), {}).setdefault(r["Counter_Name"], {})
        d[r["Dispatch_Id"]] = d.get(r["Dispatch_Id"], 0.0) + float(r["Counter_Value"])
res = {}
for k, counters in sorted(per.items()):
    row = {c: {"per_launch_mean": sum(v.values()) / len(v), "per_launch_min": min(v.values()), "per_launch_max": max(v.values()),
               "launches": len(v)} for c, v in counters.items()}
    mean = {c: row[c]["per_launch_mean"] for c in row}
    if "GRBM_GUI_ACTIVE" in mean:
        clocks = mean["GRBM_GUI_ACTIVE"] / 8
        row["clocks"] = clocks
        if "SQ_WAVE_CYCLES" in mean:
            row["occupied"] = 4 * mean["SQ_WAVE_CYCLES"] / (4096 * clocks)
        if "SQ_BUSY_CYCLES" in mean:
            row["se_busy"] = mean["SQ_BUSY_CYCLES"] / 32 / clocks
        if "SQ_ACTIVE_INST_VALU" in mean:
            row["valu_busy"] = 4 * mean["SQ_ACTIVE_INST_VALU"] / (1024 * clocks)
    res[k] = row
    print(k, {n: round(v, 4) for n, v in row.items() if not isinstance(v, dict)})
json.dump(res, open(out, "w"), indent=1)
