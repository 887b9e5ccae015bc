"""Time of one EDM2Precond.jvp call (fg_edm2_jvp) beside one forward() call (fg_edm2_forward) of the same build: EDM2-S
(EDM2_IN64_S_Config, seeded random weights) on one GPU in the bf16x3 and bf16 compute modes.  Device events around each call; after a
warm-up of both, `--rounds` rounds alternate `--calls` forwards and `--calls` jvps; reported: median (min, max) per mode.  Prints one
JSON line (and writes it to --out).

    python scripts/edm2_jvp_bench.py [--batch 64] [--rounds 4] [--calls 3] [--out profiles/edm2_jvp_in64_s_b64.json]

For a per-kernel table run it under the kernel trace with one mode, one round and the jvp alone:

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/edm2_jvp_bench.py --modes bf16x3 --rounds 1 --calls 2 --only jvp"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fastgen_amd.networks.EDM2.network import EDM2Precond  # noqa: E402

import edm2_ref as D  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["bf16x3", "bf16"])
    ap.add_argument("--only", choices=["forward", "jvp"], default=None, help="time one of the two alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    cfg, B = D.IN64_S, a.batch
    sd = D.random_state_dict(cfg, seed=1234)
    g = torch.Generator().manual_seed(5)
    t = torch.exp(torch.linspace(-1.5, 1.0, B, dtype=torch.float64))
    x = (torch.randn(B, 3, 64, 64, generator=g) * (0.25 + t ** 2).sqrt().float().reshape(-1, 1, 1, 1)).to(dev)
    vx = torch.randn(B, 3, 64, 64, generator=g).to(dev)
    vt = (0.5 * t).float().to(dev)
    lab = torch.nn.functional.one_hot(torch.arange(B) * 7 % 1000, 1000).float().to(dev)
    t = t.to(dev)
    res = {"workload": "EDM2Precond EDM2-S in64, one call", "batch": B, "rounds": a.rounds, "calls_per_round": a.calls}
    for mode in a.modes:
        net = EDM2Precond(**cfg.kwargs(), compute_dtype=mode)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).eval().requires_grad_(False)
        fwd = lambda: net(x, t, condition=lab)  # noqa: E731
        jvp = lambda: net.jvp(x, t, vx, vt, condition=lab)  # noqa: E731
        tf, tj = [], []
        with torch.no_grad():
            for _ in range(2):
                o = fwd() if a.only != "jvp" else None
                o2, j = jvp() if a.only != "forward" else (None, None)
            torch.cuda.synchronize()
            if a.only is None:
                assert torch.equal(o, o2) and torch.isfinite(j).all()
            for _ in range(a.rounds):
                if a.only != "jvp":
                    tf += [timed(fwd) for _ in range(a.calls)]
                if a.only != "forward":
                    tj += [timed(jvp) for _ in range(a.calls)]
        r = {}
        if tf:
            r.update(forward_ms=round(statistics.median(tf), 2), forward_min_max_ms=[round(min(tf), 2), round(max(tf), 2)])
        if tj:
            r.update(jvp_ms=round(statistics.median(tj), 2), jvp_min_max_ms=[round(min(tj), 2), round(max(tj), 2)])
        if tf and tj:
            r["ratio"] = round(statistics.median(tj) / statistics.median(tf), 3)
        res[mode] = r
        del net
        torch.cuda.empty_cache()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
