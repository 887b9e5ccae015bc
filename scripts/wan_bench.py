"""Time the causal video DiT at the reference's Self-Forcing / CausVid shape (fastgen/configs/experiments/WanT2V/config_sf.py:21,43:
Wan2.1-T2V-1.3B, latents [16, 21, 60, 104] = 480p, chunk of 3 frames, t_list of 4 steps): one network call of the student loop on
chunk k (4680 query tokens over (3 k + 3) * 1560 cached + own keys), and the whole 21-frame 4-step loop (7 chunks x (4 + 1) calls).
Random-init weights of the 1.3B architecture, synthetic latents and text embeddings.
    python scripts/wan_bench.py [--layers=30] [--loop] [--compute-dtype=bf16[,fp8]] [--case=chunks|bc|guided] [--chunks=0,6]
                                [--widths=1.3b|14b] [--trace=CALLS] [--bidirectional] [--i2v] [--vace] [--ti2v [--first-frame=both|yes|no]]
--vace (with --bidirectional): the video-to-video network `VACEWan` (fastgen_amd/networks/VaceWan/network.py: a VACE block behind every
  second layer, a 96-channel control video of 21 frames) next to `Wan` of the same widths and depth in the same run, at [1,16,21,60,104]:
  one forward, the 4-step x0 student loop (one hipGraph), one fg_wan_set_vace_context, and the tiled 96-channel patch embedding against
  the per-output kernel (fg_op_wan_vace_patch_embed path 2 vs 1) on that context.  The expected ratio of the forwards is
  (layers + VACE layers) / layers plus one D x D injection GEMM per VACE layer.  --trace=CALLS: one arm, `VACEWan` alone, one warm-up +
  CALLS forwards and nothing else, for `rocprofv3 --kernel-trace --stats`.
--ti2v: Wan2.2-TI2V-5B (configs/experiments/Wan{T2V,I2V}/config_*_wan22_5b.py: 24 heads x 128, 48 latent channels, ffn 14336, 30 layers)
  on latents [1, 48, 21, 44, 80] (18 480 tokens): one forward and the 2-step x0 student loop t_list = [0.999, 0.833, 0.0] (one hipGraph)
  per arm, as the text-to-video network `Wan(expand_timesteps=True)` ("no first frame") and as the image-to-video network
  `WanI2V(concat_mask=False, ...)` ("first frame").  Random weights, no checkpoint, parity unpinned.  --trace=CALLS: one arm, one
  network (--first-frame=yes|no), one warm-up + CALLS forwards and nothing else, for `rocprofv3 --kernel-trace --stats`.
--i2v (with --bidirectional): the image-to-video network `WanI2V` (fastgen_amd/networks/WanI2V/network.py: 36 input channels, 257 CLIP
  image tokens of width 1280) next to `Wan` of the same widths and depth in the same run, one call at [1,16,21,60,104] each: the cost of
  the image branch (the dual cross-attention, the two-source patch embedding) is the difference of the two numbers.  Also the call
  without image tokens, and the condition's own cost (fg_wan_set_i2v_cond, once per condition).  --trace=CALLS: one arm, `WanI2V` alone,
  one warm-up + CALLS forwards and nothing else, for `rocprofv3 --kernel-trace --stats`.
--bidirectional: the bidirectional network `Wan` (fastgen_amd/networks/Wan/network.py) instead, per arm next to the block-causal call of
  a `CausalWan` of the same weights in the same run: one call at [1,16,21,60,104] (full attention: 7 / 4 of the block mask's key
  pairs), the 4-step x0 student loop (FastGenModel.generator_fn, one hipGraph) and one guided step (the call at the stacked batch 2).
--compute-dtype: the arms (default bf16).  Several arms are built on the same seed and timed SIDE BY SIDE in this one run: per shape
  three rounds of windows, the arms alternating inside a round, the median window per arm reported (and their ratio).
--case: chunks (default) - one call per listed chunk (default all 7) over the cache the earlier chunks' calls left; bc - the all-frames
  block-causal call (32 760 tokens); guided - the chunk calls at the stacked batch 2 of the guided teacher sampler ([cond; neg]).
--widths=14b: inner dim 5120, ffn 13 824 (Wan2.1-T2V-14B's; --layers defaults to 2 then: the weights of 40 layers are 56 GB of fp32).
--trace=CALLS: for `rocprofv3 --kernel-trace`: ONE arm, the listed chunks, one warm-up + CALLS calls each, nothing else (scripts/
  wan_linear_trace.py reads the per-linear times out of the trace)."""
import statistics
import sys
import time

import torch

from fastgen_amd.methods.distribution_matching.causvid import CausVidModel
from fastgen_amd.networks.Wan.network_causal import CausalWan


def _opt(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith(f"--{name}=")), default)


WIDTHS = _opt("widths", "1.3b")
LAYERS = int(_opt("layers", "30" if WIDTHS == "1.3b" else "2"))
ARMS = _opt("compute-dtype", "bf16").split(",")
CASE = _opt("case", "chunks")
CHUNKS = [int(c) for c in _opt("chunks", "0,1,2,3,4,5,6").split(",")]
TRACE = int(_opt("trace", "0"))
TI2V = "--ti2v" in sys.argv
FIRST_FRAME = _opt("first-frame", "both")
assert FIRST_FRAME in ("both", "yes", "no") and (not (TI2V and TRACE) or FIRST_FRAME != "both")
if TI2V and not any(a.startswith("--layers=") for a in sys.argv[1:]):
    LAYERS = 30
assert WIDTHS in ("1.3b", "14b") and CASE in ("chunks", "bc", "guided") and all(a in ("bf16", "fp8") for a in ARMS) and (not TRACE or len(ARMS) == 1)
H, Fd = (12, 8960) if WIDTHS == "1.3b" else (40, 13824)
D, fs, Lt = H * 128, 1560, 512
B = 2 if CASE == "guided" else 1

nets = {}
for arm in ([] if "--i2v" in sys.argv or "--vace" in sys.argv or TI2V else ARMS):
    torch.manual_seed(0)  # the same weights in every arm
    nets[arm] = CausalWan(num_attention_heads=H, ffn_dim=Fd, num_layers=LAYERS, compute_dtype=arm).cuda().eval()
x = torch.randn(B, 16, 21, 60, 104, device="cuda")
text = torch.randn(B, Lt, 4096, device="cuda")
t = torch.tensor([0.7] * B, dtype=torch.float64, device="cuda")


def gflop(L, Lkv):
    return B * LAYERS * (2 * L * D * (4 * D + 2 * Fd + 2 * D) + 4 * L * Lkv * D + 4 * L * Lt * D) / 1e9


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def side_by_side(label, fns, n, gf=None, rounds=3):
    """fns: {arm: callable}; every arm warmed, then `rounds` rounds of one n-call window per arm, alternating."""
    for fn in fns.values():
        fn()
    times = {a: [] for a in fns}
    for _ in range(rounds):
        for a, fn in fns.items():
            times[a].append(window(fn, n))
    med = {a: statistics.median(v) for a, v in times.items()}
    parts = [f"{a} {med[a] * 1e3:8.2f} ms (min {min(times[a]) * 1e3:.2f}, max {max(times[a]) * 1e3:.2f})" +
             (f" {gf / med[a] / 1e3:6.1f} TFLOP/s" if gf else "") for a in fns]
    ratio = f"   bf16 / fp8 = {med['bf16'] / med['fp8']:.3f}" if "bf16" in med and "fp8" in med else ""
    print(f"{label}: " + "   ".join(parts) + ratio, flush=True)
    return med


if TI2V:
    from fastgen_amd.methods.model import FastGenModel
    from fastgen_amd.networks.Wan.network import Wan
    from fastgen_amd.networks.WanI2V.network import WanI2V

    KW5B = dict(num_attention_heads=24, attention_head_dim=128, in_channels=48, out_channels=48, ffn_dim=14336, num_layers=LAYERS)
    x5 = torch.randn(1, 48, 21, 44, 80, device="cuda")
    ff5 = torch.randn(1, 48, 1, 44, 80, device="cuda")
    text1, t1 = text[:1], t[:1]
    print(f"Wan2.2-TI2V-5B widths, {LAYERS} layers, latents {tuple(x5.shape)}, 18480 tokens: random weights, no checkpoint, parity unpinned")
    for arm in ARMS:
        for first in (("no", "yes") if FIRST_FRAME == "both" else (FIRST_FRAME,)):
            torch.manual_seed(0)
            if first == "yes":
                net = WanI2V(concat_mask=False, use_image_encoder=False, expand_timesteps=True, image_dim=None, compute_dtype=arm, **KW5B)
                cond = {"text_embeds": text1, "first_frame_cond": ff5}
            else:
                net = Wan(expand_timesteps=True, compute_dtype=arm, **KW5B)
                cond = text1
            net = net.cuda().eval()
            with torch.inference_mode():
                fwd = lambda: net(x5, t1, condition=cond, fwd_pred_type="flow")  # noqa: E731
                if TRACE:
                    window(fwd, 1 + TRACE)
                else:
                    label = f"{arm}, {'first frame' if first == 'yes' else 'no first frame'}"
                    side_by_side(f"{label}: one forward", {arm: fwd}, 2)
                    side_by_side(f"{label}: 2-step x0 student loop (2 network calls, one graph)",
                                 {arm: lambda: FastGenModel.generator_fn(net, x5, student_sample_steps=2, t_list=[0.999, 0.833, 0.0], condition=cond,
                                                                         student_sample_type="sde", seed=1)}, 2)
            del net
            torch.cuda.empty_cache()
    sys.exit(0)

if "--bidirectional" in sys.argv and "--i2v" in sys.argv:
    from fastgen_amd.networks.Wan.network import Wan
    from fastgen_amd.networks.WanI2V.network import WanI2V

    x1, text1, t1, L = x[:1], text[:1], t[:1], 21 * fs
    ff = torch.randn(1, 16, 21, 60, 104, device="cuda")
    img = torch.randn(1, 257, 1280, device="cuda")
    cond, cond_noimg = ({"text_embeds": text1, "first_frame_cond": ff, "encoder_hidden_states_image": img},
                        {"text_embeds": text1, "first_frame_cond": ff})
    for arm in ARMS:
        torch.manual_seed(0)
        plain = None if TRACE else Wan(num_attention_heads=H, ffn_dim=Fd, num_layers=LAYERS, compute_dtype=arm).cuda().eval()
        i2v = WanI2V(num_attention_heads=H, ffn_dim=Fd, num_layers=LAYERS, image_dim=1280, compute_dtype=arm).cuda().eval()
        with torch.inference_mode():
            if TRACE:
                window(lambda: i2v(x1, t1, condition=cond, fwd_pred_type="flow"), 1 + TRACE)
                break
            med = side_by_side(f"{arm}: one call, {L} tokens, {LAYERS} layers, {WIDTHS}",
                               {"Wan": lambda: plain(x1, t1, condition=text1, fwd_pred_type="flow"),
                                "WanI2V": lambda: i2v(x1, t1, condition=cond, fwd_pred_type="flow"),
                                "WanI2V, no image tokens": lambda: i2v(x1, t1, condition=cond_noimg, fwd_pred_type="flow")}, 2)
            print(f"   image branch: {(med['WanI2V'] - med['Wan']) * 1e3:.2f} ms per call = {(med['WanI2V'] - med['Wan']) / LAYERS * 1e6:.0f} us per "
                  f"layer ({(med['WanI2V'] / med['Wan'] - 1) * 100:.1f} %); without image tokens {(med['WanI2V, no image tokens'] - med['Wan']) * 1e3:+.2f} ms")

            def set_cond():  # a fresh condition every time: embed the image, project it per block
                i2v._slots["i2v"].forget()
                i2v._prepare(x1, "x_t", ff, img)
            side_by_side(f"{arm}: fg_wan_set_i2v_cond (257 image tokens, {LAYERS} layers)", {"set": set_cond}, 3)
            del plain, i2v
    sys.exit(0)

if "--bidirectional" in sys.argv and "--vace" in sys.argv:
    from fastgen_amd import _lib
    from fastgen_amd.methods.model import FastGenModel
    from fastgen_amd.networks._engine import ptr
    from fastgen_amd.networks.VaceWan.network import VACEWan
    from fastgen_amd.networks.Wan.network import Wan

    x1, text1, t1, L = x[:1], text[:1], t[:1], 21 * fs
    ctx = torch.cat([torch.randn(1, 32, 21, 60, 104, device="cuda"), torch.ones(1, 64, 21, 60, 104, device="cuda")], dim=1)
    cond = {"text_embeds": text1, "vid_context": ctx}
    vace_layers = list(range(0, LAYERS, 2))
    for arm in ARMS:
        torch.manual_seed(0)
        vace = VACEWan(num_attention_heads=H, ffn_dim=Fd, num_layers=LAYERS, vace_layers=vace_layers, compute_dtype=arm).cuda().eval()
        plain = None if TRACE else Wan(num_attention_heads=H, ffn_dim=Fd, num_layers=LAYERS, compute_dtype=arm).cuda().eval()
        with torch.inference_mode():
            if TRACE:
                window(lambda: vace(x1, t1, condition=cond, fwd_pred_type="flow"), 1 + TRACE)
                sys.exit(0)
            nv = len(vace_layers)
            expect = (LAYERS + nv) / LAYERS
            med = side_by_side(f"{arm}: one forward, {L} tokens, {LAYERS} layers + {nv} VACE blocks, {WIDTHS}",
                               {"Wan": lambda: plain(x1, t1, condition=text1, fwd_pred_type="flow"),
                                "VACEWan": lambda: vace(x1, t1, condition=cond, fwd_pred_type="flow")}, 2)
            print(f"   VACEWan / Wan = {med['VACEWan'] / med['Wan']:.3f} (blocks alone: {expect:.3f}; + {nv} injection GEMMs of "
                  f"{2 * L * D * D / 1e9:.0f} GFLOP each)")
            loop = lambda net, c: FastGenModel.generator_fn(net, x1, student_sample_steps=4, t_list=[0.999, 0.937, 0.833, 0.624, 0.0],  # noqa: E731
                                                            condition=c, student_sample_type="sde", seed=1)
            med = side_by_side(f"{arm}: 4-step x0 student loop (4 network calls, one graph)",
                               {"Wan": lambda: loop(plain, text1), "VACEWan": lambda: loop(vace, cond)}, 1)
            print(f"   VACEWan / Wan = {med['VACEWan'] / med['Wan']:.3f}")

            def set_ctx():  # a fresh context every time: embed it, pad it, proj_in
                vace._slots["vace"].forget()
                vace._prepare(x1, "x_t", ctx)
            side_by_side(f"{arm}: fg_wan_set_vace_context (21 context frames)", {"set": set_ctx}, 3)
            del plain, vace
            torch.cuda.empty_cache()
    with torch.inference_mode():
        w = torch.randn(D, 96, 1, 2, 2, device="cuda") * 384 ** -0.5
        b = torch.zeros(D, device="cuda")
        out = torch.empty(1, L, D, dtype=torch.bfloat16, device="cuda")
        op = lambda path: _lib.check(_lib.lib().fg_op_wan_vace_patch_embed(ptr(ctx), ptr(w), ptr(b), ptr(out), 1, 96, 21, 60, 104, D, path, None))  # noqa: E731
        med = side_by_side(f"96-channel patch embedding, {L} tokens, D {D}", {"generic": lambda: op(1), "tiled": lambda: op(2)}, 5)
        print(f"   generic / tiled = {med['generic'] / med['tiled']:.2f}")
    sys.exit(0)

if "--bidirectional" in sys.argv:
    from fastgen_amd.methods.model import FastGenModel
    from fastgen_amd.networks.Wan.network import Wan

    full = {}
    for arm in ARMS:
        torch.manual_seed(0)
        full[arm] = Wan(num_attention_heads=H, ffn_dim=Fd, num_layers=LAYERS, compute_dtype=arm).cuda().eval()
    x1, text1, t1, L = x[:1], text[:1], t[:1], 21 * fs
    x2, text2, t2 = x1.repeat(2, 1, 1, 1, 1), torch.cat([text1, -text1]), t1.repeat(2)
    tf = torch.full((1, 21), 0.7, dtype=torch.float64, device="cuda")
    B = 1
    with torch.inference_mode():
        fns = {}
        for a in ARMS:
            fns[f"{a} full"] = lambda n=full[a]: n(x1, t1, condition=text1, fwd_pred_type="flow")
            fns[f"{a} block-causal"] = lambda n=nets[a]: n(x1, tf, condition=text1, fwd_pred_type="flow", is_ar=False)
        med = side_by_side(f"one call, {L} tokens, {LAYERS} layers", fns, 2)
        print("   " + "   ".join(f"{a}: full / block-causal = {med[f'{a} full'] / med[f'{a} block-causal']:.3f}" for a in ARMS) +
              f"   (attention key pairs 7 / 4; GEMM + other work equal; full call {gflop(L, L):.0f} GFLOP, block-causal {gflop(L, L * 4 // 7):.0f})")
        loop = lambda net: FastGenModel.generator_fn(net, x1, student_sample_steps=4, t_list=[0.999, 0.937, 0.833, 0.624, 0.0],  # noqa: E731
                                                     condition=text1, student_sample_type="sde", seed=1)
        side_by_side("4-step x0 student loop (4 network calls, one graph)", {a: (lambda n=n: loop(n)) for a, n in full.items()}, 1)
        B = 2
        side_by_side("guided step: one call at the stacked batch 2", {a: (lambda n=n: n(x2, t2, condition=text2, fwd_pred_type="flow"))
                                                                       for a, n in full.items()}, 2, gflop(L, L))
    sys.exit(0)

with torch.inference_mode():
    if CASE == "bc":
        tf = torch.full((B, 21), 0.7, dtype=torch.float64, device="cuda")
        call = lambda net: net(x, tf, condition=text, fwd_pred_type="flow", is_ar=False)  # noqa: E731
        if TRACE:
            window(lambda: call(nets[ARMS[0]]), 1 + TRACE)
        else:
            L = 21 * fs
            # (keys per query under the block mask: on average 4 of the 7 chunks)
            side_by_side(f"block-causal call, {L} tokens, {LAYERS} layers", {a: (lambda n=n: call(n)) for a, n in nets.items()}, 2,
                         gflop(L, L * 4 // 7))
    else:
        for k in range(max(CHUNKS) + 1):  # fill the caches chunk by chunk, timing the call on the listed chunks
            xs = x[:, :, 3 * k: 3 * k + 3]
            call = lambda net: net(xs, t, condition=text, cur_start_frame=3 * k, store_kv=True, is_ar=True)  # noqa: E731
            if k not in CHUNKS:
                for net in nets.values():
                    call(net)
            elif TRACE:
                window(lambda: call(nets[ARMS[0]]), 1 + TRACE)
            else:
                side_by_side(f"chunk {k} (batch {B}, {LAYERS} layers, {WIDTHS})", {a: (lambda n=n: call(n)) for a, n in nets.items()}, 3,
                             gflop(3 * fs, (3 * k + 3) * fs))
    if "--loop" in sys.argv and not TRACE:
        noise = torch.randn(1, 16, 21, 60, 104, device="cuda")
        text1 = text[:1]
        loop = lambda net: CausVidModel.generator_fn(net, noise.clone(), student_sample_steps=4, t_list=[0.999, 0.937, 0.833, 0.624, 0.0],  # noqa: E731
                                                     condition=text1)
        med = side_by_side("21-frame 4-step CausVid loop (35 network calls)", {a: (lambda n=n: loop(n)) for a, n in nets.items()}, 1)
        print("   " + "   ".join(f"{a}: {21 / v:.2f} latent frames / s" for a, v in med.items()))
