"""Per-linear kernel times of the causal video DiT out of a `rocprofv3 --kernel-trace` of scripts/wan_bench.py --trace=CALLS:
    rocprofv3 --kernel-trace --output-format csv -d out/wan_trace_fp8 -o t -- python3 scripts/wan_bench.py --layers=2 \
        --compute-dtype=fp8 --chunks=6 --trace=3
    python scripts/wan_linear_trace.py out/wan_trace_fp8 --layers=2 --calls=3 --fill=6 [--warm=1]
(--fill: the untimed calls that fill the caches of the chunks before the first listed one.)
The token GEMM's kernels carry no linear's name, so a launch is attributed by its position: fg_wan_set_text launches 2 + layers GEMMs
(once, before the first call), then every block launches its six block linears in the order qkv, attn1.to_out, attn2.to_q, attn2.to_out,
ffn.net.0, ffn.net.2.  A split-K finishing pass is added to the GEMM before it; an activation quantiser (fp8 mode: the bf16 form of
quant_rows_fp8_kernel) is reported beside the GEMM after it, which reads its output.  Printed per linear: mean microseconds over the
timed calls (the warm-up calls of every listed chunk are dropped) - GEMM, quantiser pass, and the LayerNorm-modulate kernels' mean."""
import csv
import glob
import sys

LINEARS = ("qkv", "attn1.to_out", "attn2.to_q", "attn2.to_out", "ffn.net.0", "ffn.net.2")


def _opt(name, default):
    return int(next((a.split("=", 1)[1] for a in sys.argv[2:] if a.startswith(f"--{name}=")), default))


def main():
    d, layers, calls, warm, fill = sys.argv[1], _opt("layers", 2), _opt("calls", 3), _opt("warm", 1), _opt("fill", 0)
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        with open(f, newline="") as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    gemms, pending_q, ln = [], 0.0, []  # gemms: [gemm us, quantiser us] per main GEMM launch, in launch order
    for s, e, name in rows:
        us = (e - s) / 1e3
        if "gemm_splitk_finish_kernel" in name:
            gemms[-1][0] += us
        elif "gemm_bf16" in name:
            gemms.append([us, pending_q])
            pending_q = 0.0
        elif "quant_rows_fp8_kernel" in name and ("IDF16b" in name or "__bf16" in name):  # (the fp32 form quantises weights at pack time)
            pending_q += us
        elif "ln_modulate_kernel" in name:
            ln.append(us)
    block = gemms[2 + layers:]
    per_call = 6 * layers
    n_calls = len(block) // per_call
    assert len(block) % per_call == 0 and n_calls >= fill and (n_calls - fill) % (warm + calls) == 0, (len(gemms), layers, calls, warm, fill)
    keep = [c for c in range(fill, n_calls) if (c - fill) % (warm + calls) >= warm]
    print(f"{len(rows)} kernels, {n_calls} network calls of {layers} layers, {len(keep)} timed; LayerNorm-modulate mean {sum(ln) / max(len(ln), 1):.1f} us")
    total = 0.0
    for i, lname in enumerate(LINEARS):
        g = [block[c * per_call + b * 6 + i] for c in keep for b in range(layers)]
        mg, mq = sum(v[0] for v in g) / len(g), sum(v[1] for v in g) / len(g)
        total += mg + mq
        print(f"  {lname:14s} GEMM {mg:8.1f} us   quantiser before it {mq:6.1f} us")
    print(f"  six linears of a block: {total:.1f} us")


if __name__ == "__main__":
    main()
