"""The image-to-video cross-attention (wan_dual_xattn_kernel, fastgen_amd/csrc/wan_i2v.hip, through fg_op_wan_dual_cross_attention)
against the composition it replaces: fa_kernel over the text keys + fa_kernel over the image keys (fg_op_attention_ex with scratch, the
launcher's own plan, as a block without the fused kernel would launch them) + a bf16 add.  Interleaved k|v operands (ldk = 2 D) as the
engine passes them.  Kernel durations come from a kernel trace, as for scripts/attn_bench.py (fg_op_attention_ex allocates and frees its
key-split scratch around the launch and drains the stream: host-side timers and device events would measure that):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 scripts/wan_dual_attn_bench.py
    python3 scripts/wan_dual_attn_bench.py --parse DIR [--json PATH]
Per shape the arms run REPS times each, one after another (dual, text, image, add); the first launch of an arm is dropped, the mean of the
rest reported; a key-split merge launch counts to the attention launch before it.  Random operands."""
import ctypes
import json
import statistics
import sys

SHAPES = [("14B widths, 480p x 21 frames", 1, 40, 32760, 512, 257), ("1.3B widths, one 3-frame chunk", 1, 12, 4680, 512, 257)]
REPS = 6

if "--parse" in sys.argv:
    import csv
    import glob

    d = sys.argv[sys.argv.index("--parse") + 1]
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    kind = lambda n: ("dual" if "wan_dual_xattn" in n else "fa" if ("fa_kernel" in n or "fa2_kernel" in n) else "combine" if "fa128_combine" in n  # noqa: E731
                      else "add" if ("elementwise" in n and "BFloat16" in n and "add" in n.lower()) else None)
    seq = [(kind(r["Kernel_Name"]), us(r)) for r in rows if kind(r["Kernel_Name"])]
    launches = []  # (arm kind, duration with its merge pass)
    for k, t in seq:
        if k == "combine":
            launches[-1] = (launches[-1][0], launches[-1][1] + t)
        else:
            launches.append((k, t))
    assert len(launches) == 4 * REPS * len(SHAPES), (len(launches), [k for k, _ in launches][:40])
    results = []
    for i, (name, B, H, Lq, Lt, Li) in enumerate(SHAPES):
        mine = launches[4 * REPS * i: 4 * REPS * (i + 1)]
        arms = {}
        for j, (arm, want) in enumerate((("dual", "dual"), ("text", "fa"), ("image", "fa"), ("add", "add"))):
            grp = mine[REPS * j: REPS * (j + 1)]
            assert all(k == want for k, _ in grp), (arm, grp)
            arms[arm] = statistics.mean(t for _, t in grp[1:])
        comp = arms["text"] + arms["image"] + arms["add"]
        gf = 4.0 * B * H * Lq * (Lt + Li) * 128 / 1e9
        print(f"{name}: B {B}, {H} heads, Lq {Lq}, L_txt {Lt}, L_img {Li}\n"
              f"   dual kernel            {arms['dual']:9.1f} us  {gf / arms['dual'] * 1e3:6.1f} TFLOP/s\n"
              f"   text + image + add     {comp:9.1f} us  = {arms['text']:.1f} + {arms['image']:.1f} + {arms['add']:.1f}\n"
              f"   dual / composition     {arms['dual'] / comp:9.3f}", flush=True)
        results.append({"shape": name, "B": B, "heads": H, "lq": Lq, "l_txt": Lt, "l_img": Li, "us": arms, "composition_us": comp,
                        "dual_over_composition": arms["dual"] / comp})
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(results, f, indent=1)
    sys.exit(0)

import torch  # noqa: E402

from fastgen_amd import _lib  # noqa: E402

L = _lib.lib()
p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
for name, B, H, Lq, Lt, Li in SHAPES:
    D = H * 128
    q = torch.randn(B, Lq, D, device="cuda").bfloat16()
    kvt = torch.randn(B, Lt, 2 * D, device="cuda").bfloat16()
    kvi = torch.zeros(B, (Li + 31) // 32 * 32, 2 * D, device="cuda").bfloat16()
    kvi[:, :Li] = torch.randn(B, Li, 2 * D, device="cuda").bfloat16()
    out, o1, o2 = (torch.empty_like(q) for _ in range(3))

    def attn(kv, Lkv, dst):
        _lib.check(L.fg_op_attention_ex(p(q), D, Lq * D, p(kv), p(kv, 2 * D), 2 * D, kv.shape[1] * 2 * D, p(dst), D, Lq * D, B, H, 128, Lq, Lkv, 1, 0, 0,
                                        stream))

    for _ in range(REPS):
        _lib.check(L.fg_op_wan_dual_cross_attention(p(q), D, Lq * D, p(kvt), p(kvt, 2 * D), 2 * D, Lt * 2 * D, Lt, p(kvi), p(kvi, 2 * D), 2 * D,
                                                    kvi.shape[1] * 2 * D, Li, p(out), D, Lq * D, B, H, Lq, stream))
    for _ in range(REPS):
        attn(kvt, Lt, o1)
    for _ in range(REPS):
        attn(kvi, Li, o2)
    for _ in range(REPS):
        torch.add(o1, o2, out=out)
    torch.cuda.synchronize()
    print(name, "done", flush=True)
