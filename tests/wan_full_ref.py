"""The bidirectional video DiT (reference fastgen/networks/Wan/network.py `Wan`) composed from the pieces of oracle/wan_ref.py - TEST
INFRASTRUCTURE ONLY.  PARITY UNPINNED like oracle/wan_ref.py: nothing here is recorded from the reference (diffusers does not import).
Added to those pieces, each from the reference's own file: the second time embedder `r_embedder` (`init_embedder`, :799-834;
`classify_forward_prepare`, :330-351, the `encoder_depth is None` branch), `skip_layers` (`classify_forward_block_forward`, :408), the
two student loops (`FastGenModel._student_sample_loop`, methods/model.py:315-372; `MeanFlowModel._student_sample_loop`,
consistency_model/mean_flow.py:336-381) on the RF schedule and the guided teacher loop `Wan.sample` (:919-988) over the solver step of
fastgen_amd/networks/Wan/solvers.py (as tests/wan_guided_ref.py).  Runs in the dtype it is given: fp32 or fp64."""
from typing import Dict, Optional

import torch

from fastgen_amd.networks.Wan import solvers
from oracle import wan_ref as R

R_KEYS = ("time_embedder.linear_1.weight", "time_embedder.linear_1.bias", "time_embedder.linear_2.weight", "time_embedder.linear_2.bias",
          "time_proj.weight", "time_proj.bias")


def state_dict_shapes(cfg: R.WanConfig, r_timestep: bool = False) -> Dict[str, tuple]:
    """`Wan.state_dict()`: CausalWan's keys, then the r_embedder's six behind logvar_linear (it is attached last, :615-619)."""
    sd = dict(R.state_dict_shapes(cfg))
    if r_timestep:
        for k in R_KEYS:
            sd["transformer.r_embedder." + k] = sd["transformer.condition_embedder." + k]
    return sd


def random_state_dict(cfg: R.WanConfig, seed: int = 0, r_timestep: bool = False, r_init: str = "random_full") -> Dict[str, torch.Tensor]:
    """`R.random_state_dict` plus the r_embedder.  r_init: "random_full" - its own draws at the scale of the t embedder's (same rule:
    fan-in scaled matrices, 0.05 biases), so that an r term of the wrong size or kind moves the output as much as a wrong t would;
    "zero" / "pretrained" - the reference's `init_embedder` modes."""
    sd = R.random_state_dict(cfg, seed)
    if not r_timestep:
        return sd
    g = torch.Generator().manual_seed(seed + 100003)
    for k in R_KEYS:
        src = sd["transformer.condition_embedder." + k]
        if r_init == "zero":
            v = torch.zeros_like(src)
        elif r_init == "pretrained":
            v = src.clone()
        elif k.endswith(".bias"):
            v = 0.05 * torch.randn(src.shape, generator=g)
        else:
            v = torch.randn(src.shape, generator=g) * src.shape[1] ** -0.5
        sd["transformer.r_embedder." + k] = v
    return sd


class WanFullRef:
    """mutant: None - the network; "ignore_r" - r is dropped; "swap_cond" - time_cond_type swapped; "proj_only" - r_timestep_proj is
    added to timestep_proj but remb is not added to temb.  The mutants are what the GPU test must tell the HIP path from."""

    def __init__(self, sd: Dict[str, torch.Tensor], cfg: R.WanConfig, dtype=torch.float32, time_cond_type: str = "diff",
                 mutant: Optional[str] = None):
        assert time_cond_type in ("diff", "abs") and mutant in (None, "ignore_r", "swap_cond", "proj_only")
        self.cfg, self.dtype, self.mutant = cfg, dtype, mutant
        self.time_cond_type = time_cond_type if mutant != "swap_cond" else {"diff": "abs", "abs": "diff"}[time_cond_type]
        self.p = {k[len("transformer."):]: v.to(dtype) for k, v in sd.items()}
        self.has_r = "r_embedder.time_proj.weight" in self.p

    def forward(self, x_t: torch.Tensor, t: torch.Tensor, text: torch.Tensor, r: Optional[torch.Tensor] = None, skip_layers=None) -> torch.Tensor:
        """The raw network output.  x_t [B, C, F, H, W]; t, r [B] in the schedule's units.  The embedders see the fp32 values 1000 t and
        1000 r (and their fp32 difference) in every dtype, as the C ABI's t_frames / r_frames."""
        cfg, p, dt = self.cfg, self.p, self.dtype
        B, C, Fr, H, W = x_t.shape
        gh, gw = H // 2, W // 2
        ts32 = (1000.0 * t.float()).view(B, 1).expand(B, Fr).reshape(-1)  # (as CausalWanRef.forward forms it)
        cos, sin = R.rope_for_chunk(cfg, Fr, gh, gw, 0, dt)
        hs = R.patch_embed(p, x_t.to(dt))
        temb = R.time_embedding(p, cfg, ts32.to(dt))
        tproj = R.time_projection(p, temb)
        if r is not None:
            if not self.has_r:
                raise ValueError("r_timestep provided but no r_embedder is present")
            if self.mutant != "ignore_r":
                rs32 = (1000.0 * r.float()).view(B, 1).expand(B, Fr).reshape(-1)
                if self.time_cond_type == "diff":
                    rs32 = ts32 - rs32
                pr = {k.replace("r_embedder.", "condition_embedder."): v for k, v in p.items() if k.startswith("r_embedder.")}
                remb = R.time_embedding(pr, cfg, rs32.to(dt))
                tproj = tproj + R.time_projection(pr, remb)
                if self.mutant != "proj_only":
                    temb = temb + remb
        ctx = R.text_embedding(p, text.to(dt))
        for i in range(cfg.num_layers):
            if skip_layers is not None and i in skip_layers:
                continue
            mod = R.modulation(p, i, tproj, B, Fr)
            q, k, v = R.self_attn_qkv(p, cfg, i, hs, mod, cos, sin)
            hs = R.self_attn_out(p, i, hs, R.sdpa(q, k, v), mod)
            k2, v2 = R.cross_kv(p, cfg, i, ctx)
            hs = R.cross_attn(p, cfg, i, hs, k2, v2)[1]
            hs = R.ffn(p, cfg, i, hs, mod)
        return R.final_layer(p, cfg, hs, temb, Fr, gh, gw)


def x0_loop(net: WanFullRef, noise: torch.Tensor, t_list: torch.Tensor, text: torch.Tensor, eps_list=None, sample_type: str = "sde"):
    """`FastGenModel.generator_fn` + `_student_sample_loop` on the RF schedule (alpha = 1 - t, sigma = t), flow-predicting network."""
    B = noise.shape[0]
    x = noise * float(t_list[0])
    draws = iter(eps_list or [])
    x0 = None
    for i in range(len(t_list) - 1):
        tc, tn = float(t_list[i]), float(t_list[i + 1])
        x0 = x - tc * net.forward(x, t_list[i].expand(B), text)
        if tn > 0:
            eps = next(draws) if sample_type == "sde" else (x - (1 - tc) * x0) / tc
            x = (1 - tn) * x0 + tn * eps
    return x0


def meanflow_loop(net: WanFullRef, noise: torch.Tensor, t_list: torch.Tensor, text: torch.Tensor, eps_list=None, sample_type: str = "sde"):
    """`MeanFlowModel._student_sample_loop`: u = net(x, t, r) with r = 0 ('sde': jump to the data end, re-noise to t_next unless it is
    0) or r = t_next ('ode': x <- x - (t - t_next) u)."""
    B = noise.shape[0]
    x = noise * float(t_list[0])
    draws = iter(eps_list or [])
    for i in range(len(t_list) - 1):
        tc, tn = float(t_list[i]), float(t_list[i + 1])
        if sample_type == "sde":
            x = x - tc * net.forward(x, t_list[i].expand(B), text, r=torch.zeros(B, dtype=t_list.dtype))
            if tn > 0:
                x = (1 - tn) * x + tn * next(draws)
        else:
            x = x - (tc - tn) * net.forward(x, t_list[i].expand(B), text, r=t_list[i + 1].expand(B))
    return x


def guided_sample(net: WanFullRef, noise, text, neg_text, guidance_scale, num_steps, shift=5.0, solver="unipc"):
    """`Wan.sample` (fp64 solver state over the network's dtype).  guidance_scale None / neg_text None: the unguided loop."""
    sig = solvers.flow_shift_sigmas(num_steps, shift)
    guided = guidance_scale is not None and neg_text is not None
    table = solvers.multistep_table(sig, solver, guidance_scale if guided else 1.0)
    t_net = torch.clamp(torch.floor(sig[:-1] * 1000.0) / 1000.0, max=0.999)
    B = noise.shape[0]
    x, x_last, m_prev = noise.double() * float(t_net[0]), None, None
    for i in range(num_steps):
        t = t_net[i].expand(B)
        v = net.forward(x.to(net.dtype), t, text).double()
        vu = net.forward(x.to(net.dtype), t, neg_text).double() if guided else None
        x, x_last, m_prev = solvers.multistep_update(table[i], x, v, x_last, m_prev, v_uncond=vu)
    return x


# ---- the cases tests/test_gpu_wan_full.py runs against this oracle; tests/test_wan_full_ref.py holds their mutants apart on the CPU ------
SHAPES = {"ragged": (2, 16, 5, 16, 24), "long": (1, 16, 12, 16, 24)}  # 480 tokens per sample x 2; 1152 tokens (> 1024 keys, > 6 frames)
R_SEED, R_T, R_R = 61, (0.8, 0.45), (0.3, 0.1)  # weights seed, t and r per sample (the first B entries)
MUTANTS = ("ignore_r", "swap_cond", "proj_only")


def r_case(shape_key: str = "ragged"):
    """(state dict with a full-scale r_embedder, x, t, r, text) of the r cases."""
    shp = SHAPES[shape_key]
    sd = random_state_dict(R.TINY, R_SEED, r_timestep=True)
    g = torch.Generator().manual_seed(R_SEED + 1)
    x = torch.randn(shp, generator=g)
    text = torch.randn(shp[0], 24, 128, generator=g)
    t = torch.tensor(R_T[: shp[0]], dtype=torch.float64)
    r = torch.tensor(R_R[: shp[0]], dtype=torch.float64)
    return sd, x, t, r, text
