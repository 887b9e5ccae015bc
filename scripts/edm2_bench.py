"""Few-step sampling throughput of EDM2Precond(**EDM2_IN64_S_Config) (EDM2-S, 280.2 M parameters) on one GPU: the fused,
graph-replayed FastGenModel.generator_fn at 1 and 4 steps in the bf16x3 and bf16 compute modes, and the torch-eager functional
restatement (tests/edm2_ref.py, fp32 torch ops on the same GPU) as a comparison arm.  Prints one JSON line.

    python scripts/edm2_bench.py [--batch 256] [--reps 3] [--eager-batch 64]

Roof fraction: 201.6 GFLOP per image per forward (torch.utils.flop_counter on the reference at B = 1, 99.4 % of it in the
convolutions) against 833 TFLOP/s (three bf16 MFMAs per product) for bf16x3 and 2.5 PFLOP/s for bf16."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fastgen_amd.methods.model import FastGenModel  # noqa: E402
from fastgen_amd.networks.EDM2.network import EDM2Precond  # noqa: E402

import edm2_ref as D  # noqa: E402

GFLOP_PER_FWD = 201.6
ROOF_TF = {"bf16x3": 833.0, "bf16": 2500.0}


def timed(fn, reps):
    fn()  # warm-up: packing, graph capture
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--eager-batch", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B = args.batch
    sd = D.random_state_dict(D.IN64_S, seed=1)
    net = EDM2Precond(**D.IN64_S.kwargs())
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(0)
    noise = torch.randn(B, 3, 64, 64, generator=g).to(dev)
    cond = torch.nn.functional.one_hot(torch.arange(B) % 1000, 1000).float().to(dev)
    res = {"workload": "EDM2Precond EDM2-S in64 generator_fn", "batch": B, "gflop_per_forward": GFLOP_PER_FWD}
    for mode in ("bf16x3", "bf16"):
        net.compute_dtype = mode
        for steps in (1, 4):
            sec = timed(lambda: FastGenModel.generator_fn(net, noise, student_sample_steps=steps, condition=cond,
                                                          student_sample_type="sde", seed=5), args.reps)
            tflops = GFLOP_PER_FWD * B * steps / sec / 1e3
            res[f"{mode}_{steps}step"] = {"ms": round(sec * 1e3, 2), "img_per_s": round(B / sec, 1), "tflops": round(tflops, 1),
                                          "roof_frac": round(tflops / ROOF_TF[mode], 4)}
    # torch-eager arm: the functional restatement, one forward, fp32 torch on the same GPU
    Be = args.eager_batch
    sdg = {k: v.to(dev) for k, v in sd.items()}
    x = noise[:Be] * 80.0
    t = torch.full((Be,), 80.0, dtype=torch.float64, device=dev)

    def eager():
        with torch.no_grad():
            D.precond_forward(sdg, D.IN64_S, x, t, cond[:Be])

    sec = timed(eager, args.reps)
    res["torch_eager_fp32_1forward"] = {"batch": Be, "ms": round(sec * 1e3, 2), "img_per_s": round(Be / sec, 1),
                                        "tflops": round(GFLOP_PER_FWD * Be / sec / 1e3, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
