"""Wan2.2 TI2V-5B's conventions (reference fastgen/networks/WanI2V/network.py `WanI2V` with concat_mask = False, use_image_encoder =
False, expand_timesteps = True; fastgen/networks/Wan/network.py `Wan` with expand_timesteps = True) composed from the pieces of
oracle/wan_ref.py the way tests/wan_full_ref.py composes `Wan` - TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED: nothing here is recorded
from the reference (diffusers does not import).  Added to those pieces, literally from the reference's own files:
  * `_replace_first_frame` (WanI2V/network.py:254-277): (1 - mask) * first_frame_cond + mask * latents with mask [1, 1, F, H, W], zero on
    frame 0;
  * `_compute_timestep_inputs` (Wan/network.py:904-917): one timestep per TOKEN, mask[:, ::1, ::2, ::2] * rescale_t(t), flattened to
    [B, seq_len]; the time embedder, time_proj, every block's modulation (`block_forward`, Wan/network.py:114-125, the temb.ndim == 4
    branch) and the output layer's then run per token;
  * `WanI2V.forward` (:457-523): convert_model_output on the CALLER's x_t and [B] t, then frame 0 of the result replaced;
  * `preserve_conditioning` (:228-252), the generic student loop with that hook (methods/model.py:315-372) and `WanI2V.sample`
    (:344-419: guided flow zeroed on frame 0, frame 0 of the latents restored after every solver step).
Runs in the dtype it is given: fp32 or fp64.  The condition is a dict {"text", "ff"} with ff [B, C, 1, H, W] (or [B, C, F, H, W])."""
import dataclasses
from typing import Dict, Optional

import torch

from fastgen_amd.networks.Wan import solvers
from oracle import wan_ref as R
import wan_full_ref as W

TINY48 = dataclasses.replace(R.TINY, in_channels=48, out_channels=48)  # D 256, 2 heads, ffn 512, 2 layers, text_dim 128
MUTANTS = ("no_input_replacement", "first_frame_t_not_zero", "no_output_replacement", "neighbour_first_frame", "convert_on_replaced_x_t")
INPUT_SIDE = ("no_input_replacement", "first_frame_t_not_zero", "neighbour_first_frame")  # measured on frames >= 1
TIME_SCALE, Q_SCALE = 4.0, 3.0


def random_state_dict(cfg: R.WanConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """`R.random_state_dict` with two groups of weights scaled, as tests/wan_i2v_ref.py scales `add_k_proj`, so that the reference alone
    holds the input-side mutants apart (frame 0's contents and timestep reach the other frames only through its self-attention keys
    and values): the time embedder's first linear x TIME_SCALE, and every block's `attn1.norm_q.weight` x Q_SCALE - at unit scale the
    self-attention logits are O(1), the softmax is close to a mean over all tokens and another first frame moves the other frames by
    1e-2 relative; three times sharper, a query picks its keys.  Distances: tests/test_wan_ti2v_ref.py."""
    sd = R.random_state_dict(cfg, seed)
    k = "transformer.condition_embedder.time_embedder.linear_1.weight"
    sd[k] = TIME_SCALE * sd[k]
    for k in sd:
        if k.endswith("attn1.norm_q.weight"):
            sd[k] = Q_SCALE * sd[k]
    return sd


def first_frame_mask(x: torch.Tensor) -> torch.Tensor:
    """[1, 1, F, H, W]: ones, zero on frame 0 (`_replace_first_frame`)."""
    m = torch.ones(1, 1, *x.shape[2:], dtype=x.dtype)
    m[:, :, 0] = 0
    return m


def replace_first_frame(ff: torch.Tensor, latents: torch.Tensor) -> torch.Tensor:
    m = first_frame_mask(latents)
    return (1 - m) * ff[:, :, :1].to(latents.dtype) + m * latents


def final_layer_per_token(p, cfg: R.WanConfig, hs: torch.Tensor, temb: torch.Tensor, Fr: int, gh: int, gw: int) -> torch.Tensor:
    """`R.final_layer` with one modulation row per token: temb [B * L, D]."""
    B, L, D = hs.shape
    so = p["scale_shift_table"].view(1, 1, 2, D) + temb.view(B, L, 1, D)
    y = R.layer_norm(hs, cfg.eps) * (1 + so[:, :, 1]) + so[:, :, 0]
    o = R._lin(p, y, "proj_out").view(B, Fr, gh, gw, 1, 2, 2, -1)
    return o.permute(0, 7, 1, 4, 2, 5, 3, 6).reshape(B, -1, Fr, 2 * gh, 2 * gw)


class WanTI2VRef:
    """i2v = True: `WanI2V` on the TI2V convention; False: `Wan(expand_timesteps=True)` (mask of ones, no replacement, cond["ff"] unread).
    per_frame_rows: the same network with one embedder row per FRAME (what the engine computes) instead of one per token.
    Mutants (what the GPU test must tell the HIP path from): "no_input_replacement" - the network reads x_t's own frame 0;
    "first_frame_t_not_zero" - a mask of ones; "no_output_replacement" - frame 0 of the result is the network's;
    "neighbour_first_frame" - sample b gets sample b + 1's first frame on the input side; "convert_on_replaced_x_t" - the replacement
    comes BEFORE the conversion, which then runs on the replaced x_t (frame 0 of an x0 result is (1 - t) ff instead of ff)."""

    def __init__(self, sd: Dict[str, torch.Tensor], cfg: R.WanConfig, dtype=torch.float32, i2v: bool = True, mutant: Optional[str] = None,
                 per_frame_rows: bool = False):
        assert mutant in (None,) + MUTANTS
        self.cfg, self.dtype, self.i2v, self.mutant, self.per_frame_rows = cfg, dtype, i2v, mutant, per_frame_rows
        self.p = {k[len("transformer."):]: v.to(dtype) for k, v in sd.items()}

    def raw(self, x_in: torch.Tensor, t: torch.Tensor, mask: torch.Tensor, text: torch.Tensor) -> torch.Tensor:
        """The transformer on its input x_in with the expanded timesteps of `mask` [1, F, H, W]."""
        cfg, p, dt = self.cfg, self.p, self.dtype
        B, _, Fr, H, W = x_in.shape
        gh, gw = H // 2, W // 2
        L = Fr * gh * gw
        t32 = 1000.0 * t.float()  # rescale_t; the embedder sees fp32 values in every dtype, as the C ABI's rows
        cos, sin = R.rope_for_chunk(cfg, Fr, gh, gw, 0, dt)
        hs = R.patch_embed(p, x_in.to(dt))
        ctx = R.text_embedding(p, text.to(dt))
        if self.per_frame_rows:
            ts = (mask[:, :, 0, 0].float() * t32.view(-1, 1)).reshape(-1)  # [B * F]
            rows = Fr
        else:
            ts = (mask[:, ::1, ::2, ::2].float() * t32.view(-1, 1, 1, 1)).flatten(1).reshape(-1)  # [B * seq_len]
            rows = L
        temb = R.time_embedding(p, cfg, ts.to(dt))
        tproj = R.time_projection(p, temb)
        for i in range(cfg.num_layers):
            mod = R.modulation(p, i, tproj, B, rows)  # [B, rows, 6, D]: the pieces below modulate `rows` groups of L / rows tokens
            q, k, v = R.self_attn_qkv(p, cfg, i, hs, mod, cos, sin)
            hs = R.self_attn_out(p, i, hs, R.sdpa(q, k, v), mod)
            k2, v2 = R.cross_kv(p, cfg, i, ctx)
            hs = R.cross_attn(p, cfg, i, hs, k2, v2)[1]
            hs = R.ffn(p, cfg, i, hs, mod)
        if self.per_frame_rows:
            return R.final_layer(p, cfg, hs, temb, Fr, gh, gw)
        return final_layer_per_token(p, cfg, hs, temb, Fr, gh, gw)

    def forward(self, x_t: torch.Tensor, t: torch.Tensor, cond: dict, r=None, fwd_pred_type: str = "flow") -> torch.Tensor:
        """`forward(x_t, t, condition, fwd_pred_type=...)` of a flow-predicting network on the RF schedule: x0 = x_t - t flow."""
        assert r is None and fwd_pred_type in ("flow", "x0")
        dt, mu = self.dtype, self.mutant
        x_t = x_t.to(dt)
        tb = t.to(dt).view(-1, 1, 1, 1, 1)
        convert = (lambda x, o: x - tb * o) if fwd_pred_type == "x0" else (lambda x, o: o)
        if not self.i2v:
            return convert(x_t, self.raw(x_t, t, torch.ones(1, *x_t.shape[2:]), cond["text"]))
        ff = cond["ff"].to(dt)
        ff_in = torch.roll(ff, -1, dims=0) if mu == "neighbour_first_frame" else ff
        x_in = x_t if mu == "no_input_replacement" else replace_first_frame(ff_in, x_t)
        mask = first_frame_mask(x_t)[:, 0]
        if mu == "first_frame_t_not_zero":
            mask = torch.ones_like(mask)
        out = self.raw(x_in, t, mask, cond["text"])
        if mu == "convert_on_replaced_x_t":
            return convert(replace_first_frame(ff, x_t), replace_first_frame(ff, out))
        out = convert(x_t, out)
        return out if mu == "no_output_replacement" else replace_first_frame(ff, out)

    def preserve_conditioning(self, x: torch.Tensor, cond: dict) -> torch.Tensor:
        if not self.i2v:
            return x
        x = x.clone()
        x[:, :, 0] = cond["ff"][:, :, 0].to(x.dtype)
        return x


def x0_loop(net: WanTI2VRef, noise: torch.Tensor, t_list: torch.Tensor, cond: dict, eps_list=None, sample_type: str = "sde"):
    """`FastGenModel._student_sample_loop` with the `preserve_conditioning` hook on every prediction and every re-noised state."""
    B = noise.shape[0]
    x = noise * float(t_list[0])
    draws = iter(eps_list or [])
    x0 = None
    for i in range(len(t_list) - 1):
        tc, tn = float(t_list[i]), float(t_list[i + 1])
        x0 = net.preserve_conditioning(net.forward(x, t_list[i].expand(B), cond, fwd_pred_type="x0"), cond)
        if tn > 0:
            eps = next(draws) if sample_type == "sde" else (x - (1 - tc) * x0) / tc
            x = net.preserve_conditioning((1 - tn) * x0 + tn * eps, cond)
    return x0


def guided_sample(net: WanTI2VRef, noise, cond, neg_cond, guidance_scale, num_steps, shift=3.0, solver="unipc"):
    """`WanI2V.sample` (fp64 solver state over the network's dtype), as tests/wan_full_ref.py's `guided_sample` with the guided flow
    zeroed on frame 0 (zero conditional and unconditional flows: the same guided flow) and frame 0 restored after every step."""
    sig = solvers.flow_shift_sigmas(num_steps, shift)
    guided = guidance_scale is not None and neg_cond is not None
    table = solvers.multistep_table(sig, solver, guidance_scale if guided else 1.0)
    t_net = torch.clamp(torch.floor(sig[:-1] * 1000.0) / 1000.0, max=0.999)
    B = noise.shape[0]
    x, x_last, m_prev = noise.double() * float(t_net[0]), None, None
    for i in range(num_steps):
        t = t_net[i].expand(B)
        v = net.forward(x.to(net.dtype), t, cond).double()
        vu = net.forward(x.to(net.dtype), t, neg_cond).double() if guided else None
        if net.i2v:
            v[:, :, 0] = 0.0
            if vu is not None:
                vu[:, :, 0] = 0.0
        x, x_last, m_prev = solvers.multistep_update(table[i], x, v, x_last, m_prev, v_uncond=vu)
        if net.i2v:
            x = x.clone()
            x[:, :, 0] = cond["ff"][:, :, 0].double()
    return x


# ---- the case tests/test_gpu_wan_ti2v.py runs; tests/test_wan_ti2v_ref.py holds its mutants apart on the CPU ----------------------------
SHAPE = (2, 48, 5, 16, 24)  # 480 tokens per sample
TEXT_LEN, SEED, T = 37, 83, (0.9, 0.9)


def case(seed: int = SEED):
    """(state dict, x, t, cond) of the forward test: first frames at the latents' scale, one per sample."""
    sd = random_state_dict(TINY48, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(SHAPE, generator=g)
    cond = {"text": torch.randn(SHAPE[0], TEXT_LEN, 128, generator=g), "ff": torch.randn(SHAPE[0], SHAPE[1], 1, *SHAPE[3:], generator=g)}
    return sd, x, torch.tensor(T, dtype=torch.float64), cond
