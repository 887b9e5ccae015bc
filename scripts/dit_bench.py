"""Time the DiT-XL/2 forward (fastgen/configs/net.py:124-127: hidden 1152, 28 blocks, 16 heads x 72, 256 tokens) on one MI355X.
Algorithmic work per image and forward: 28 x (qkv 2.04 + attention 0.30 + proj 0.68 + MLP 5.44) GFLOP + embeddings = 237 GFLOP.
    python scripts/dit_bench.py [--mode=bf16x3|bf16|fp8[,mode ...]] [--pairs=N] [--json=PATH] [--input-size=32|64[,...]] [batch ...]
--input-size=64 is the 512 x 512 model (1024 tokens: attention 4.83 GFLOP per block and image, 1006 GFLOP per image and forward);
`--input-size=64,32 64 256` times B 64 at 64 beside B 256 at 32 - the i-th batch goes with the i-th size, interleaved in every round.
Several comma-separated modes share one module (one engine per mode) and are timed interleaved, --pairs rounds each (A / B runs on one
chip state: `--mode=bf16,fp8 --pairs=4 256`); --json writes every round's time.
    python scripts/dit_bench.py --jvp [--pairs=N] [--json=PATH] [batch ...]
times `DiT.jvp` (the MeanFlow tangent; bf16x3, r_timestep, 256 tokens) beside the bf16x3 forward of the same module, interleaved in
every round, at B = 8 (the per-GPU batch of the reference's MeanFlow-XL config) and B = 64 by default.  The comparison points are that
forward and twice that forward - what the reference's finite-difference alternative (use_jvp_finite_diff) costs."""
import json
import sys
import time

import torch

from fastgen_amd.networks.DiT.network import DiT

MODES = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--mode=")), "bf16x3").split(",")
PAIRS = next((int(a.split("=", 1)[1]) for a in sys.argv[1:] if a.startswith("--pairs=")), 1)
JSON = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--json=")), None)
SIZES = [int(v) for v in next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--input-size=")), "32").split(",")]
D, depth, Hd = 1152, 28, 4608


def gflop(T):
    return depth * (2 * T * D * 3 * D + 4 * T * T * D + 2 * T * D * D + 4 * T * D * Hd + 2 * D * 6 * D) / 1e9


if "--jvp" in sys.argv[1:]:
    net = DiT(compute_dtype="bf16x3", r_timestep=True, time_cond_type="diff", scale_t=False).cuda().eval()
    with torch.no_grad():
        g = torch.Generator().manual_seed(0)
        for n, p in net.named_parameters():
            p.copy_((torch.randn(p.shape, generator=g) * (0.1 if p.dim() == 1 else p.shape[-1] ** -0.5)).cuda())
    rounds, ratios = [], {}
    for B in [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [8, 64]:
        x, vx = torch.randn(B, 4, 32, 32, device="cuda"), torch.randn(B, 4, 32, 32, device="cuda")
        t = torch.rand(B, device="cuda") * 0.9 + 0.05
        r, one, zero = t * 0.5, torch.ones(B, device="cuda"), torch.zeros(B, device="cuda")
        c = torch.randint(0, 1000, (B,), device="cuda")
        arms = {"forward": lambda: net(x, t, condition=c, r=r), "jvp": lambda: net.jvp(x, t, vx, one, condition=c, r=r, v_r=zero)}
        with torch.inference_mode():
            for fn in arms.values():
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            n = 4 if B >= 32 else 16
            for rnd in range(PAIRS):
                ms = {}
                for name, fn in arms.items():
                    fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        fn()
                    torch.cuda.synchronize()
                    ms[name] = (time.perf_counter() - t0) / n * 1e3
                    rounds.append({"batch": B, "round": rnd, "call": name, "ms": ms[name]})
                ratios.setdefault(B, []).append(ms["jvp"] / ms["forward"])
                print(f"B={B:4d} round {rnd}: forward {ms['forward']:8.2f} ms  jvp {ms['jvp']:8.2f} ms  jvp / forward {ms['jvp'] / ms['forward']:.2f} "
                      f"(finite difference: 2.00)", flush=True)
    if JSON:
        with open(JSON, "w") as f:
            json.dump({"mode": "bf16x3", "rounds": rounds, "jvp_over_forward": {str(b): sorted(v)[len(v) // 2] for b, v in ratios.items()}}, f, indent=1)
    sys.exit(0)

nets = {}
for size in SIZES:
    if size in nets:
        continue
    nets[size] = DiT(input_size=size, compute_dtype=MODES[0]).cuda().eval()
    with torch.no_grad():
        g = torch.Generator().manual_seed(0)
        for n, p in nets[size].named_parameters():  # O(1) signal in every branch (the reference zero-initialises the adaLN layers)
            p.copy_((torch.randn(p.shape, generator=g) * (0.1 if p.dim() == 1 else p.shape[-1] ** -0.5)).cuda())
    T = (size // 2) ** 2
    print(f"input_size {size}: compute mode {', '.join(MODES)}; {gflop(T):.1f} GFLOP / image / forward, attention {100 * depth * 4 * T * T * D / 1e9 / gflop(T):.1f} % of it")
rounds = []
BATCHES = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [64, 256]
if len(SIZES) > 1:  # paired (batch, size) arms, all interleaved in each round
    assert len(SIZES) == len(BATCHES), "--input-size=a,b needs one batch per size"
    arms = []
    for B, size in zip(BATCHES, SIZES):
        arms.append((B, size, torch.randn(B, 4, size, size, device="cuda"), torch.rand(B, dtype=torch.float64, device="cuda") * 0.99,
                     torch.randint(0, 1000, (B,), device="cuda")))
    with torch.inference_mode():
        for B, size, x, t, c in arms:
            for mode in MODES:
                nets[size].compute_dtype = mode
                for _ in range(2):
                    nets[size](x, t, condition=c)
        torch.cuda.synchronize()
        for rnd in range(PAIRS):
            for mode in MODES:
                for B, size, x, t, c in arms:
                    net = nets[size]
                    net.compute_dtype = mode
                    net(x, t, condition=c)
                    torch.cuda.synchronize()
                    t0, n = time.perf_counter(), 4
                    for _ in range(n):
                        net(x, t, condition=c)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) / n
                    GF = gflop((size // 2) ** 2)
                    rounds.append({"batch": B, "input_size": size, "round": rnd, "mode": mode, "ms": dt * 1e3, "img_per_s": B / dt,
                                   "algorithmic_tflops": B * GF / dt / 1e3})
                    print(f"input_size {size} B={B:4d} {mode:7s}: {dt * 1e3:8.2f} ms / forward  {B / dt:8.1f} img/s  {B * GF / dt / 1e3:7.1f} algorithmic TFLOP/s",
                          flush=True)
    BATCHES = []
net, GF = nets[SIZES[0]], gflop((SIZES[0] // 2) ** 2)
for B in BATCHES:
    x = torch.randn(B, 4, SIZES[0], SIZES[0], device="cuda")
    t = torch.rand(B, dtype=torch.float64, device="cuda") * 0.99
    c = torch.randint(0, 1000, (B,), device="cuda")
    with torch.inference_mode():
        for mode in MODES:  # pack and warm every engine before the first timed round
            net.compute_dtype = mode
            for _ in range(2):
                net(x, t, condition=c)
        torch.cuda.synchronize()
        for rnd in range(PAIRS):
            for mode in MODES:
                net.compute_dtype = mode
                net(x, t, condition=c)
                torch.cuda.synchronize()
                t0, n = time.perf_counter(), 4
                for _ in range(n):
                    net(x, t, condition=c)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / n
                rounds.append({"batch": B, "round": rnd, "mode": mode, "ms": dt * 1e3, "img_per_s": B / dt})
                print(f"B={B:4d} {mode:7s}: {dt * 1e3:8.2f} ms / forward  {B / dt:8.1f} img/s  {B * GF / dt / 1e3:7.1f} algorithmic TFLOP/s", flush=True)
if JSON:
    with open(JSON, "w") as f:
        json.dump({"gflop_per_image": {str(size): gflop((size // 2) ** 2) for size in SIZES}, "rounds": rounds}, f, indent=1)
