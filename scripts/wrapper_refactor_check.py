"""Identity check for changes to the four network wrappers (EDMPrecond, EDM2Precond, DiT, CausalWan) that must not change what they
build or compute.  Run it at two commits and compare the files it writes: they must be byte-identical.

    python scripts/wrapper_refactor_check.py --out construct.txt          # no GPU: seeded construction of every wrapper
    python scripts/wrapper_refactor_check.py --gpu --out outputs.txt      # + a SHA-256 of every output of a list of small calls
    python scripts/wrapper_refactor_check.py --host-time                  # host time per call of two overhead-bound forwards

Construction: after torch.manual_seed(0), the ordered state-dict keys (buffers included) and the named_parameters() order, each with
shape, dtype and a SHA-256 of the tensor's bytes.  --gpu: seeded weights and inputs at the smallest shapes the engines accept.
--host-time measures HOST OVERHEAD (bind check, workspace lookup, marshalling, launches) at B = 2 / B = 3, not kernel speed."""
import argparse
import hashlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fastgen_amd.networks.DiT.network import DiT  # noqa: E402
from fastgen_amd.networks.EDM.network import EDMPrecond  # noqa: E402
from fastgen_amd.networks.EDM2.network import EDM2Precond  # noqa: E402
from fastgen_amd.networks.Wan.network_causal import CausalWan  # noqa: E402

SONG = dict(img_resolution=32, img_channels=3, label_dim=10, sigma_shift=0.0, sigma_data=0.5, model_type="SongUNet", augment_dim=9,
            model_channels=128, channel_mult=[2, 2, 2], channel_mult_noise=1, embedding_type="positional", encoder_type="standard",
            decoder_type="standard", resample_filter=[1, 1], dropout=0.0, label_dropout=0, r_timestep=False, drop_precond=None)
SONG_MF = dict(SONG, r_timestep=True, drop_precond="both", schedule_type="rf", net_pred_type="flow")
ADM = dict(img_resolution=64, img_channels=3, label_dim=10, sigma_shift=0.0, sigma_data=0.5, model_type="DhariwalUNet", augment_dim=9,
           model_channels=64, channel_mult=[1, 2, 3, 4], channel_mult_emb=4, num_blocks=1, attn_resolutions=[32, 16, 8], dropout=0.0,
           label_dropout=0, r_timestep=False, drop_precond=None)
EDM2 = dict(img_resolution=64, img_channels=3, label_dim=10, model_channels=64, channel_mult=[1, 2, 3, 4], num_blocks=1,
            attn_resolutions=[16, 8], label_balance=0.5, concat_balance=0.5, res_balance=0.3, attn_balance=0.3, clip_act=256,
            logvar_channels=128, sigma_data=0.5)
DIT_S = dict(hidden_size=384, depth=2, num_heads=6)
WAN = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2, chunk_size=2, total_num_frames=6)

BUILDERS = [
    ("song", lambda: EDMPrecond(**SONG)), ("song_r", lambda: EDMPrecond(**SONG_MF)), ("adm", lambda: EDMPrecond(**ADM)),
    ("edm2", lambda: EDM2Precond(**EDM2)), ("dit_s16", lambda: DiT(input_size=32, **DIT_S)), ("dit_s32", lambda: DiT(input_size=64, **DIT_S)),
    ("wan", lambda: CausalWan(**WAN)), ("wan_nologvar", lambda: CausalWan(enable_logvar_linear=False, **WAN)),
]


def sha(t: torch.Tensor) -> str:
    b = t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(b).hexdigest()


def line(case, key, t):
    return f"{case}\t{key}\t{tuple(t.shape)}\t{t.dtype}\t{sha(t)}"


def construction():
    out = []
    for tag, make in BUILDERS:
        torch.manual_seed(0)
        net = make()
        out += [line(tag + ".state_dict", k, v) for k, v in net.state_dict().items()]
        out += [line(tag + ".named_parameters", k, v) for k, v in net.named_parameters()]
        out.append(f"{tag}.modules\t{len(list(net.modules()))}")
    return out


def seeded(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


@torch.no_grad()
def randomize(net, seed):
    g = torch.Generator().manual_seed(seed)
    for p in net.parameters():
        p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return net


class Recorder:
    def __init__(self):
        self.lines = []

    def __call__(self, case, res):
        flat = []

        def walk(r):
            if isinstance(r, torch.Tensor):
                flat.append(r)
            elif r is not None:
                for x in r:
                    walk(x)

        walk(res)
        torch.cuda.synchronize()
        self.lines += [line(case, str(i), t) for i, t in enumerate(flat)]
        print(f"{case}: {len(flat)} tensors", flush=True)


def gpu_edm(rec, dev):
    x, t = seeded((2, 3, 32, 32), 1).to(dev), torch.tensor([1.0, 2.5], dtype=torch.float64, device=dev)
    cond = torch.nn.functional.one_hot(torch.arange(2) % 10, 10).float().to(dev)
    tl = [2.5, 0.8, 0.0]
    net = EDMPrecond(**SONG).randomize_parameters_(3).to(dev).eval()
    with torch.inference_mode():
        for mode in ("fp32", "bf16x3"):
            net.compute_dtype = mode
            rec(f"song.forward.{mode}", net(x, t, cond))
        net.compute_dtype = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            rec("song.forward.autocast_bf16", net(x, t, cond))
        rec("song.forward.taps", net(x, t, cond, feature_indices={0, 1}))
        rec("song.jvp", net.jvp(x, t, seeded((2, 3, 32, 32), 2).to(dev), torch.ones(2, device=dev), condition=cond))
        for graph in (True, False):
            rec(f"song.few_step.x0.graph{int(graph)}", net.few_step_sample(x, cond, tl, sample_type="sde", seed=7, use_graph=graph))
    # one training forward + backward (bf16x3)
    xg = x.clone().requires_grad_(True)
    out = net(xg, t, cond)
    out.square().sum().backward()
    named = [(n, p) for n, p in net.named_parameters() if p.grad is not None]
    rec("song.train.bf16x3", [out, xg.grad] + [named[i][1].grad for i in (0, len(named) // 2, len(named) - 1)])
    net.zero_grad(set_to_none=True)
    # mode and weight changes on one module object
    with torch.inference_mode(False), torch.no_grad():
        net.compute_dtype = "fp32"
        a = net(x, t, cond)
        net.compute_dtype = "bf16x3"
        rec("song.change.mode", [a, net(x, t, cond)])
        net.model._modules["enc"]._modules["32x32_block1"]._modules["conv0"].weight.add_(0.01)
        rec("song.change.add_", net(x, t, cond))
        fresh = EDMPrecond(**SONG).randomize_parameters_(11)
        net.load_state_dict(fresh.state_dict())
        rec("song.change.load_state_dict", net(x, t, cond))
        net.to(torch.bfloat16)
        rec("song.change.to_bf16", net(x, t, cond))
    del net, fresh
    mf = EDMPrecond(**SONG_MF).randomize_parameters_(4).to(dev).eval()
    tm, rm = torch.tensor([0.9, 0.6], dtype=torch.float64, device=dev), torch.tensor([0.4, 0.1], dtype=torch.float64, device=dev)
    with torch.inference_mode():
        rec("song_r.forward", mf(x, tm, cond, r=rm))
        rec("song_r.few_step.meanflow", mf.few_step_sample(x, cond, [0.999, 0.5, 0.0], sample_type="ode", seed=7))
    del mf
    adm = EDMPrecond(**ADM).randomize_parameters_(5).to(dev).eval()
    xa = seeded((2, 3, 64, 64), 6).to(dev)
    with torch.inference_mode():
        rec("adm.forward", adm(xa, t, cond))
        rec("adm.few_step.x0", adm.few_step_sample(xa, cond, tl, sample_type="sde", seed=7))
    del adm
    torch.manual_seed(0)
    e2 = EDM2Precond(**EDM2).to(dev).eval()
    with torch.inference_mode():
        rec("edm2.forward.bf16x3", e2(xa, t, cond))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            rec("edm2.forward.autocast_bf16", e2(xa, t, cond))
        rec("edm2.few_step.x0", e2.few_step_sample(xa, cond, tl, sample_type="sde", seed=7))


def gpu_dit(rec, dev):
    B = 3
    x, t = seeded((B, 4, 32, 32), 1).to(dev), torch.tensor([0.9, 0.5, 0.2], device=dev)
    cls, neg = torch.tensor([1, 7, 999], device=dev), torch.full((B,), 1000, device=dev)
    torch.manual_seed(0)
    net = randomize(DiT(input_size=32, **DIT_S), 3).to(dev).eval()
    with torch.inference_mode():
        for mode in ("fp32", "bf16x3", "bf16", "fp8"):
            net.compute_dtype = mode
            rec(f"dit.forward.{mode}", net(x, t, cls))
        net.compute_dtype = None
        rec("dit.forward.taps", net(x, t, cls, feature_indices={0, 1}))
        rec("dit.forward.early", net(x, t, cls, feature_indices={0}, return_features_early=True))
        rec("dit.jvp", net.jvp(x, t, seeded((B, 4, 32, 32), 2).to(dev), torch.ones(B, device=dev), condition=cls))
        rec("dit.few_step.x0", net.few_step_sample(x, cls, [0.999, 0.5, 0.0], sample_type="sde", seed=7, loop="x0"))
        rec("dit.few_step.euler_guided", net.few_step_sample(x, cls, [0.999, 0.5, 0.0], sample_type="ode", seed=7, loop="euler",
                                                              neg_condition=neg, guidance_scale=2.0))
    del net
    torch.manual_seed(0)
    netr = randomize(DiT(input_size=32, r_timestep=True, **DIT_S), 4).to(dev).eval()
    with torch.inference_mode():
        rec("dit_r.few_step.meanflow", netr.few_step_sample(x, cls, [0.999, 0.5, 0.0], sample_type="ode", seed=7, loop="meanflow"))
    del netr
    torch.manual_seed(0)
    net32 = randomize(DiT(input_size=64, compute_dtype="bf16", **DIT_S), 5).to(dev).eval()
    with torch.inference_mode():
        rec("dit_s32.forward.bf16", net32(seeded((B, 4, 64, 64), 6).to(dev), t, cls))


def gpu_wan(rec, dev):
    x = seeded((1, 16, 6, 8, 8), 1).to(dev)
    text, negt = seeded((1, 16, 128), 2).to(dev), seeded((1, 16, 128), 3).to(dev)
    for mode in ("bf16", "fp8"):
        net = CausalWan(compute_dtype=mode, **WAN).to(dev).eval()
        t0, t1 = torch.zeros(1, dtype=torch.float64, device=dev), torch.full((1,), 0.6, dtype=torch.float64, device=dev)
        with torch.inference_mode():
            a = net(x[:, :, 0:2], t0, condition=text, fwd_pred_type="flow", cur_start_frame=0, store_kv=True, is_ar=True)
            b = net(x[:, :, 2:4], t1, condition=text, fwd_pred_type="flow", cur_start_frame=2, is_ar=True)
            rec(f"wan.{mode}.ar_chunks", [a, b])
            net.clear_caches()
            rec(f"wan.{mode}.block_causal", net(x, t1, condition=text, fwd_pred_type="flow", is_ar=False))
            rec(f"wan.{mode}.student_sample", net.student_sample(x[:, :, :4].clone(), [0.9, 0.5, 0.0], text, sample_type="sde", seed=5))
            rec(f"wan.{mode}.sample_guided", net.sample(x[:, :, :4].clone(), text, negt, guidance_scale=3.0, sample_steps=2, seed=3))
        del net


def host_time(dev):
    """Median over 5 rounds of the host time per call (200 calls ending in a synchronise) of two overhead-bound forwards."""
    x, t = seeded((2, 3, 32, 32), 1).to(dev), torch.tensor([1.0, 2.5], dtype=torch.float64, device=dev)
    cond = torch.nn.functional.one_hot(torch.arange(2) % 10, 10).float().to(dev)
    edm = EDMPrecond(**SONG).randomize_parameters_(3).to(dev).eval()
    xd, td, cls = seeded((3, 4, 32, 32), 1).to(dev), torch.tensor([0.9, 0.5, 0.2], device=dev), torch.tensor([1, 7, 999], device=dev)
    dit = randomize(DiT(input_size=32, hidden_size=384, depth=12, num_heads=6), 3).to(dev).eval()
    res = {}
    with torch.inference_mode():
        for tag, call in (("edm_song_b2_forward", lambda: edm(x, t, cond)), ("dit_s_b3_forward", lambda: dit(xd, td, cls))):
            for _ in range(30):
                call()
            torch.cuda.synchronize()
            rounds = []
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(200):
                    call()
                torch.cuda.synchronize()
                rounds.append((time.perf_counter() - t0) / 200 * 1e6)
            res[tag] = statistics.median(rounds)
    print("HOST_TIME_US " + " ".join(f"{k}={v:.2f}" for k, v in res.items()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--host-time", action="store_true")
    a = ap.parse_args()
    if a.host_time:
        return host_time(torch.device("cuda:0"))
    lines = construction()
    if a.gpu:
        rec, dev = Recorder(), torch.device("cuda:0")
        gpu_edm(rec, dev)
        gpu_dit(rec, dev)
        gpu_wan(rec, dev)
        lines += rec.lines
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(f"{len(lines)} lines, sha256 {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main()
