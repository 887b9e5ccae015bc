"""Time the guided teacher sampler of the causal video DiT (`CausalWan.sample`) at the 1.3B widths on latents [1, 16, 21, 60, 104]
(480p, 7 chunks of 3 frames), 4 solver steps, classifier-free guidance - three ways, alternated in one process:
  fused      `CausalWan.sample`: one library call, per chunk and step ONE network call of the stacked batch 2 + one elementwise pass
  per-call   the reference's shape of the loop: per step two batch-1 `CausalWan.forward` calls under the cache tags "pos" / "neg", the
             guidance and solver step through the torch mirror (solvers.multistep_update), and two cache-fill calls per chunk
  unguided   `CausalWan.student_sample` with 4 steps ('ode'): what the network could run before there was guidance (the baseline)
Each is warmed up once (graph capture, allocations), then timed `--reps` times with a host clock around work that ends in a device
synchronise; the median and the spread are printed, then one JSON line.  Random-init weights, synthetic latents and text embeddings.
    python scripts/wan_guided_bench.py [--layers=30] [--reps=3] [--steps=4]"""
import json
import statistics
import sys
import time

import torch

from fastgen_amd.networks.Wan import solvers
from fastgen_amd.networks.Wan.network_causal import CausalWan


def _arg(name, default):
    return next((int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith(f"--{name}=")), default)


LAYERS, REPS, STEPS = _arg("layers", 30), _arg("reps", 3), _arg("steps", 4)
G, SHIFT, Lt = 5.0, 5.0, 512


def per_call(net, x, cond, neg):
    sig = solvers.flow_shift_sigmas(STEPS, SHIFT)
    tab = solvers.multistep_table(sig, "unipc", G)
    t_net = (torch.floor(sig[:-1] * 1000.0) / 1000.0).cuda()
    t0 = torch.zeros(1, dtype=torch.float64, device="cuda")
    net.clear_caches()
    for a in range(0, x.shape[2], net.chunk_size):
        b = a + net.chunk_size
        cur, x_last, m_prev = x[:, :, a:b], None, None
        for i in range(STEPS):
            kw = dict(fwd_pred_type="flow", cur_start_frame=a, store_kv=False, is_ar=True)
            vc = net(cur, t_net[i:i + 1], condition=cond, cache_tag="pos", **kw)
            vu = net(cur, t_net[i:i + 1], condition=neg, cache_tag="neg", **kw)
            cur, x_last, m_prev = solvers.multistep_update(tab[i], cur, vc, x_last, m_prev, v_uncond=vu)
        x[:, :, a:b] = cur
        for tag, text in (("pos", cond), ("neg", neg)):
            net(cur, t0, condition=text, cache_tag=tag, fwd_pred_type="flow", cur_start_frame=a, store_kv=True, is_ar=True)
    net.clear_caches()
    return x


def main():
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    net = CausalWan(num_layers=LAYERS).cuda().eval()
    g = torch.Generator().manual_seed(0)
    noise = torch.randn(1, 16, 21, 60, 104, generator=g).cuda()
    cond, neg = torch.randn(1, Lt, 4096, generator=g).cuda(), torch.randn(1, Lt, 4096, generator=g).cuda()
    tl = solvers.flow_shift_sigmas(STEPS, SHIFT).clamp(max=0.999)
    runs = {
        "fused": lambda: net.sample(noise.clone(), cond, neg, guidance_scale=G, sample_steps=STEPS, shift=SHIFT),
        "per_call": lambda: per_call(net, noise.clone(), cond, neg),
        "unguided": lambda: net.student_sample(noise.clone(), tl, cond, sample_type="ode"),
    }
    times = {k: [] for k in runs}
    with torch.inference_mode():
        outs = {}
        for k, fn in runs.items():  # warm-up: every shape and graph the timed window uses
            outs[k] = fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["fused"], outs["per_call"]))
        rel = float((outs["fused"] - outs["per_call"]).norm() / outs["per_call"].norm())
        for _ in range(REPS):
            for k, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:9s}: median {med[k]:.3f} s  (min {min(v):.3f}, max {max(v):.3f}, {REPS} runs)", flush=True)
    print(f"fused == per-call bit for bit: {same} (rel L2 {rel:.2e}); fused / unguided = {med['fused'] / med['unguided']:.2f}, "
          f"per-call / unguided = {med['per_call'] / med['unguided']:.2f}")
    print(json.dumps({"layers": LAYERS, "steps": STEPS, "reps": REPS, "seconds": med, "all": times, "fused_equals_per_call": same, "rel_l2": rel,
                      "fused_over_unguided": med["fused"] / med["unguided"], "per_call_over_unguided": med["per_call"] / med["unguided"]}))


if __name__ == "__main__":
    main()
