"""Summarise the rocprofv3 output of scripts/collect_profiles.sh into the files committed under profiles/:
   <tag>_kernel_stats.csv (per-kernel totals) and <tag>_pmc_dominant_kernel.json (counters of the dominant kernel,
   HBM traffic per launch with the gfx950 FETCH_SIZE correction of MI355X_MICROARCH.md)."""
import csv, glob, json, os, re, sys
from collections import defaultdict

out, tag = sys.argv[1], sys.argv[2]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the dominant kernel = the 3x3 conv at 32x32 without resampling, as a substring of the demangled name:
#   bf16x3 (headline): conv_fused_kernel<bf16x3, 3, 2, 0, 5, 0, 0>     bf16: conv3_ws_kernel<0, 5, 0, 4, 2>
DOM = sys.argv[3] if len(sys.argv) > 3 else "conv_fused_kernel<bf16x3, 3, 2, 0, 5, 0, 0>"
MODE = sys.argv[4] if len(sys.argv) > 4 else "bf16x3"


def short(n):
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    return re.sub(r"\s+", " ", n)[:120]


# kernel stats
rows = defaultdict(lambda: [0, 0.0])
for f in glob.glob(os.path.join(out, "stats", "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        k = short(r["Kernel_Name"])
        rows[k][0] += 1
        rows[k][1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
tot = sum(v[1] for v in rows.values())
with open(os.path.join(root, "profiles", f"{tag}_kernel_stats.csv"), "w") as fh:
    fh.write("kernel,calls,total_us,avg_us,percent\n")
    for k, (c, t) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
        fh.write(f"\"{k}\",{c},{t:.1f},{t / c:.2f},{100 * t / tot:.2f}\n")

# counters of the dominant kernel
cnt = defaultdict(lambda: [0, 0.0])
for f in glob.glob(os.path.join(out, "pmc*", "**", "*counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        if DOM in short(r["Kernel_Name"]):
            c = cnt[r["Counter_Name"]]
            c[0] += 1
            c[1] += float(r["Counter_Value"])
avg = {k: v[1] / v[0] for k, v in cnt.items() if v[0]}
dom = [v for k, v in rows.items() if DOM in k]
res = {
    "kernel": DOM + (f" (dominant kernel of bench.py, {MODE}, batch 512)" if len(sys.argv) <= 5 else f" ({sys.argv[5]})"),
    "command": "scripts/collect_profiles.sh: rocprofv3 --kernel-trace --pmc <group> --output-format csv -- " +
               (f"python3 bench.py --full --dtype {MODE} --steps 2 --warmup 1 --no-cpu-baseline --no-secondary" if len(sys.argv) <= 5 else sys.argv[5]) +
               " (one run per counter group)",
    "dispatches_per_pass": {k: v[0] for k, v in cnt.items()},
    "avg_launch_us_kernel_trace": (dom[0][1] / dom[0][0]) if dom else None,
    "counters_avg_per_dispatch": avg,
}
if "FETCH_SIZE" in avg and "WRITE_SIZE" in avg:
    # rocprofv3 reports FETCH_SIZE / WRITE_SIZE in KiB
    fetch_b, write_b = avg["FETCH_SIZE"] * 1024, avg["WRITE_SIZE"] * 1024
    res["FETCH_SIZE_bytes_raw"] = fetch_b
    res["WRITE_SIZE_bytes"] = write_b
    res["fetch_correction"] = "x2: on gfx950 FETCH_SIZE counts 128-B requests at 64 B for 16-B/lane coalesced streams (MI355X_MICROARCH.md, HBM section)"
    res["hbm_bytes_per_launch"] = 2 * fetch_b + write_b
if "SQ_VALU_MFMA_BUSY_CYCLES" in avg and "GRBM_GUI_ACTIVE" in avg:
    # busy cycles summed over 1024 SIMDs vs. shader-engine-active cycles (GRBM_GUI_ACTIVE is summed over the 8 XCDs)
    res["mfma_pipe_busy_frac"] = avg["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024 * avg["GRBM_GUI_ACTIVE"] / 8)
    if dom:
        res["effective_clock_GHz"] = avg["GRBM_GUI_ACTIVE"] / 8 / (dom[0][1] / dom[0][0]) / 1e3
json.dump(res, open(os.path.join(root, "profiles", f"{tag}_pmc_dominant_kernel.json"), "w"), indent=1)
print(json.dumps(res, indent=1)[:1500])
