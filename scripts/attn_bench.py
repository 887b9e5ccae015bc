"""Attention kernel (fa_kernel, fastgen_amd/csrc/wan.hip) at the shapes of the transformer rows, one shape after another so that a
`rocprofv3 --kernel-trace` of this script gives per-shape kernel durations (fg_op_attention allocates and frees its key-split scratch
around the launch: host-side timers would measure that):
    rocprofv3 --kernel-trace --output-format csv -d gpurun_out/attn -- python3 scripts/attn_bench.py
    python3 scripts/attn_bench.py --parse gpurun_out/attn      # per-shape table from the trace
Shapes: video DiT 1.3B self-attention of chunk k (4680 queries over 1560 * 3 (k + 1) keys, 12 heads x 128), its cross-attention (512 text
keys), DiT-XL/2 (B = 256, 16 heads x 72, 256 tokens).

    python3 scripts/attn_bench.py --dit [--json PATH]
times the DiT engine's own two attention kernels through fg_op_dit_attention (no allocation inside: device events around the launches):
dit_flash_kernel at B 64 x 1024 tokens against dit_attention_kernel at B 256 x 256 tokens (the same token count, 4 x the FLOPs), 16 heads,
per mode (bf16, bf16x3) and head dim (64, 72); for bf16 at head dim 72 also fa_kernel<72> on the 1024-token shape.  All arms interleaved in
one process, ROUNDS rounds of LAUNCHES launches each after a warm-up, random operands; the median round per arm.  Share of roof: of the
2.5 PFLOP/s dense bf16 MFMA rate, a third of it in the split-bf16 mode (three MFMAs per product)."""
import ctypes
import os
import glob
import sys

SHAPES = [("wan self chunk 0", 1, 12, 128, 4680, 4680), ("wan self chunk 3", 1, 12, 128, 4680, 4 * 4680), ("wan self chunk 6", 1, 12, 128, 4680, 7 * 4680),
          ("wan cross (text)", 1, 12, 128, 4680, 512), ("wan teacher-forcing chunk 6 of B=2", 2, 12, 128, 4680, 7 * 4680),
          ("DiT-XL/2 B=256", 256, 16, 72, 256, 256), ("DiT-XL/2 B=64", 64, 16, 72, 256, 256)]
REPS = 4
if os.environ.get("ATTN_SHAPES"):  # e.g. ATTN_SHAPES=2 : only "wan self chunk 6" (counter passes)
    SHAPES = [SHAPES[int(i)] for i in os.environ["ATTN_SHAPES"].split(",")]

if "--pmc" in sys.argv:  # per-kernel counter averages of a `rocprofv3 --pmc ... --output-format csv` directory
    import csv
    from collections import defaultdict

    d = sys.argv[sys.argv.index("--pmc") + 1]
    acc, cnt = defaultdict(float), defaultdict(int)
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if any(n in r["Kernel_Name"] for n in ("fa_kernel", "fa2_kernel", "fa72_seq_kernel")):
                key = (r["Kernel_Name"].split("(")[0][-40:], r["Counter_Name"])
                acc[key] += float(r["Counter_Value"])
                cnt[key] += 1
    for key in sorted(acc):
        print(f"{key[0]:42s} {key[1]:28s} {acc[key] / cnt[key]:16.0f}  (n={cnt[key]})")
    sys.exit(0)

if "--parse" in sys.argv:
    import csv

    d = sys.argv[sys.argv.index("--parse") + 1]
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    fa = [r for r in rows if any(n in r["Kernel_Name"] for n in ("fa_kernel", "fa2_kernel", "fa72_seq_kernel"))]
    cb = [r for r in rows if "fa128_combine" in r["Kernel_Name"]]
    assert len(fa) == REPS * len(SHAPES), (len(fa), len(SHAPES))
    ci = 0
    for i, (name, B, H, hd, Lq, Lkv) in enumerate(SHAPES):
        mine = fa[i * REPS + 1:(i + 1) * REPS]
        us = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in mine) / len(mine) / 1e3
        # a combine launch directly after an fa launch belongs to it
        extra = 0.0
        for r in mine:
            nxt = [c for c in cb if int(c["Start_Timestamp"]) >= int(r["End_Timestamp"])]
            later_fa = [x for x in fa if int(x["Start_Timestamp"]) > int(r["Start_Timestamp"])]
            if nxt and (not later_fa or int(nxt[0]["Start_Timestamp"]) < int(later_fa[0]["Start_Timestamp"])):
                extra += (int(nxt[0]["End_Timestamp"]) - int(nxt[0]["Start_Timestamp"])) / 1e3
        extra /= len(mine)
        gf = 4.0 * B * H * Lq * Lkv * hd / 1e9
        print(f"{name:38s} fa {us:9.1f} us (+ combine {extra:6.1f})  {gf:8.1f} GFLOP  {gf / (us + extra) * 1e3:7.1f} TFLOP/s  "
              f"{100 * gf / (us + extra) * 1e3 / 2500:5.1f} % of 2.5 PF")
    sys.exit(0)

import torch

from fastgen_amd import _lib
if os.environ.get("FA_TIMING_LIB") == "1":  # scripts/fa_ablate.sh: the FASTGEN_AMD_FA_ABL switches exist only in the timing library
    _lib.LIB_PATH = _lib.LIB_PATH.replace("libfastgen_amd.so", "libfastgen_amd_timing.so")

if os.environ.get("FA_LIB"):  # an experimental build of the library (absolute or repo-relative path)
    _lib.LIB_PATH = os.path.abspath(os.environ["FA_LIB"])

L = _lib.lib()
p = lambda t: ctypes.c_void_p(t.data_ptr())

if "--dit" in sys.argv:
    import json
    import statistics

    ROUNDS, LAUNCHES, H = 5, 4, 16
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    arms = []  # (name, mode, hd, launch, GFLOP, roof in TFLOP/s)

    def dit_arm(mode, hd, B, T, path):
        n = B * H * T * hd
        lo_off = n + 32 * T
        x3 = mode == "bf16x3"
        bufs = []
        for _ in range(3):  # q, k, vt: random hi plane (and a lo plane 2^-9 below it), 32 rows of slack behind each
            t = torch.randn(lo_off * (2 if x3 else 1), device="cuda")
            if x3:
                t[lo_off:] *= 2.0 ** -9
            bufs.append(t.bfloat16())
        out = torch.empty(B, T, H * hd, dtype=torch.float32 if x3 else torch.bfloat16, device="cuda")
        m = _lib.FG_DTYPE_BF16X3 if x3 else _lib.FG_DTYPE_BF16

        def launch():
            _lib.check(L.fg_op_dit_attention(m, p(bufs[0]), p(bufs[1]), p(bufs[2]), p(out), B, H, hd, T, lo_off if x3 else 0, path, stream))
        kernel = "dit_flash_kernel" if path == 2 else "dit_attention_kernel"
        arms.append((f"{kernel}<{mode}, {hd}> B {B} T {T}", mode, hd, launch, 4.0 * B * H * T * T * hd / 1e9, 2500.0 / (3 if x3 else 1), (bufs, out)))

    for mode in ("bf16", "bf16x3"):
        for hd in (64, 72):
            dit_arm(mode, hd, 64, 1024, 2)
            dit_arm(mode, hd, 256, 256, 1)
    B, T, hd = 64, 1024, 72
    qkv = torch.randn(B, T, 3 * H * hd, device="cuda").bfloat16()  # token-major q | k | v as the engine's bf16 path at head dim 72 keeps them
    fo = torch.empty(B, T, H * hd, dtype=torch.bfloat16, device="cuda")
    D = H * hd

    def fa72():
        _lib.check(L.fg_op_attention_ex(p(qkv), 3 * D, T * 3 * D, ctypes.c_void_p(qkv.data_ptr() + 2 * D), ctypes.c_void_p(qkv.data_ptr() + 4 * D),
                                        3 * D, T * 3 * D, p(fo), D, T * D, B, H, hd, T, T, 0, 0, 0, stream))
    arms.append((f"fa_kernel<72> (launch_fa) B {B} T {T}", "bf16", 72, fa72, 4.0 * B * H * T * T * hd / 1e9, 2500.0, (qkv, fo)))

    for a in arms:  # warm-up: code objects, clocks
        for _ in range(3):
            a[3]()
    torch.cuda.synchronize()
    times = {a[0]: [] for a in arms}
    for _ in range(ROUNDS):
        for a in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                a[3]()
            e1.record()
            e1.synchronize()
            times[a[0]].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    res = []
    for name, mode, hd, _, gf, roof, _ in arms:
        us = statistics.median(times[name])
        res.append({"arm": name, "mode": mode, "head_dim": hd, "us": us, "us_rounds": times[name], "gflop": gf, "tflops": gf / us * 1e3,
                    "roof_tflops": roof, "share_of_mfma_roof": gf / us * 1e3 / roof})
        print(f"{name:52s} {us:9.1f} us (rounds {min(times[name]):.1f} .. {max(times[name]):.1f})  {gf:8.1f} GFLOP  {gf / us * 1e3:7.1f} TFLOP/s  "
              f"{100 * gf / us * 1e3 / roof:5.1f} % of the mode's MFMA roof", flush=True)
    ratios = {}
    for mode in ("bf16", "bf16x3"):
        for hd in (64, 72):
            fl = next(r for r in res if r["arm"].startswith("dit_flash") and r["mode"] == mode and r["head_dim"] == hd)
            wh = next(r for r in res if r["arm"].startswith("dit_attention") and r["mode"] == mode and r["head_dim"] == hd)
            ratios[f"{mode}/{hd}"] = fl["tflops"] / wh["tflops"]
            print(f"flash / whole-sequence FLOP/s  {mode:7s} hd {hd}: {ratios[f'{mode}/{hd}']:.3f}")
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump({"rounds": ROUNDS, "launches_per_round": LAUNCHES, "arms": res, "flash_over_whole_sequence": ratios}, f, indent=1)
    sys.exit(0)
for name, B, H, hd, Lq, Lkv in SHAPES:
    q = torch.randn(B, Lq, H * hd, device="cuda").bfloat16()
    k = torch.randn(B, Lkv, H * hd, device="cuda").bfloat16()
    v = torch.randn(B, Lkv, H * hd, device="cuda").bfloat16()
    out = torch.empty_like(q)
    for _ in range(REPS):
        _lib.check(L.fg_op_attention(p(q), p(k), p(v), p(out), B, H, hd, Lq, Lkv, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    print(name, "done", flush=True)
