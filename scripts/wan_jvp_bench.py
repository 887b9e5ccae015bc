"""Time of one Wan.jvp call (fg_wan_jvp) beside one Wan.forward call (fg_wan_forward_full) of the same build: the bidirectional video DiT
at the Wan2.1-T2V-1.3B widths (12 heads x 128, ffn 8960, text 512 x 4096) with the r_embedder, seeded random weights, B 1, at the 480p
shape of the reference's WanT2V/config_mf.py (21 x 60 x 104 latents = 21 x 30 x 52 tokens) and at one small shape (5 x 16 x 24
latents = 480 tokens).  Device events around each call; after a warm-up of both, `--rounds` rounds alternate `--calls` forwards and
`--calls` jvps; reported: median (min, max) per shape and jvp / forward.  Prints one JSON line (and writes it to --out).

    python scripts/wan_jvp_bench.py [--layers 30] [--rounds 3] [--calls 2] [--out profiles/wan_jvp_1p3b.json]

For a per-kernel table run it under the kernel trace with one shape, one round and the jvp alone:

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/wan_jvp_bench.py --shapes 480p --rounds 1 --calls 1 --only jvp"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fastgen_amd.networks.Wan.network import Wan  # noqa: E402

SHAPES = {"480p": (21, 60, 104), "small": (5, 16, 24)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--only", choices=["forward", "jvp"], default=None, help="time one of the two alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    net = Wan(num_layers=a.layers, r_timestep=True, time_cond_type="diff", r_embedder_init="random").to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(5)
    text = torch.randn(1, 512, 4096, generator=g).to(dev)
    t, r = torch.tensor([0.8], device=dev), torch.tensor([0.3], device=dev)
    one, zero = torch.ones(1, device=dev), torch.zeros(1, device=dev)
    res = {"workload": "Wan (1.3B widths, r_embedder) one call, B 1", "layers": a.layers, "rounds": a.rounds, "calls_per_round": a.calls}
    for name in a.shapes:
        Fr, H, W = SHAPES[name]
        x, vx = torch.randn(1, 16, Fr, H, W, generator=g).to(dev), torch.randn(1, 16, Fr, H, W, generator=g).to(dev)
        fwd = lambda: net(x, t, condition=text, r=r)  # noqa: E731
        jvp = lambda: net.jvp(x, t, vx, one, condition=text, r=r, v_r=zero)  # noqa: E731
        tf, tj = [], []
        with torch.no_grad():
            for _ in range(2):
                if a.only != "jvp":
                    fwd()
                if a.only != "forward":
                    _, j = jvp()
            torch.cuda.synchronize()
            if a.only != "forward":
                assert torch.isfinite(j).all()
            for _ in range(a.rounds):
                if a.only != "jvp":
                    tf += [timed(fwd) for _ in range(a.calls)]
                if a.only != "forward":
                    tj += [timed(jvp) for _ in range(a.calls)]
        rr = {"tokens": Fr * (H // 2) * (W // 2)}
        if tf:
            rr.update(forward_ms=round(statistics.median(tf), 2), forward_min_max_ms=[round(min(tf), 2), round(max(tf), 2)])
        if tj:
            rr.update(jvp_ms=round(statistics.median(tj), 2), jvp_min_max_ms=[round(min(tj), 2), round(max(tj), 2)])
        if tf and tj:
            rr["ratio"] = round(statistics.median(tj) / statistics.median(tf), 3)
        res[name] = rr
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
