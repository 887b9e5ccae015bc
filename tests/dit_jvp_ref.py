"""fp64 mirror of the DiT forward-mode derivative (fastgen_amd/csrc/dit_jvp.hip, engine_dit.inc `dit_jvp`): the same functions, a primal
and a tangent value side by side, each citing the reference lines it follows (fastgen/networks/DiT/network.py, as oracle/dit_ref.py).
tests/test_dit_jvp_ref.py pins every function against `torch.func.jvp` of the corresponding oracle function and a central difference;
the GPU tests compare the kernels against these functions per token row and per (sample, head).

The `drop_*` switches leave terms of the derivative out.  They exist for the discrimination checks of tests/test_gpu_dit_jvp.py (a
bound is worth something only if a pass without the term misses it) and are never set otherwise."""
import math
from typing import Optional

import torch
import torch.nn.functional as F

from oracle import dit_ref as R

Tensor = torch.Tensor


def fourier_jvp(t: Tensor, td: Tensor, dim: int = 256, max_freq: float = 10000.0):
    """FourierTimeEmbedding.encode_timesteps, :67-96: f = [cos(t w) | sin(t w)], fd = [-w sin(t w) | w cos(t w)] td."""
    half = dim // 2
    w = torch.exp(-math.log(max_freq) * torch.arange(0, half, dtype=t.dtype) / half)
    ang = t[:, None] * w[None, :]
    c, s = torch.cos(ang), torch.sin(ang)
    wd = w[None, :] * td[:, None]
    return torch.cat([c, s], dim=-1), torch.cat([-s * wd, c * wd], dim=-1)


def silu_jvp(v: Tensor, vd: Tensor):
    """silu(v) = v sig(v); silu'(v) = sig (1 + v (1 - sig))."""
    sig = torch.sigmoid(v)
    return v * sig, sig * (1 + v * (1 - sig)) * vd


def time_embedding_jvp(sd, prefix: str, t: Tensor, td: Tensor):
    """FourierTimeEmbedding.forward, :98-101: Linear -> SiLU -> Linear; the tangent passes the linears without their biases."""
    f, fd = fourier_jvp(t, td)
    w0, b0, w2, b2 = (sd[prefix + k] for k in (".proj_net.0.weight", ".proj_net.0.bias", ".proj_net.2.weight", ".proj_net.2.bias"))
    h, hd = silu_jvp(F.linear(f, w0, b0), F.linear(fd, w0))
    return F.linear(h, w2, b2), F.linear(hd, w2)


def ln_modulate_jvp(x: Tensor, xd: Tensor, shift: Tensor, shiftd: Tensor, scale: Tensor, scaled: Tensor, drop_mod_tangent: bool = False):
    """LayerNorm(eps 1e-6, no affine, :167, 171, 212) + apply_adaptive_modulation (:29-41) on [B, N, D] tokens with [B, D] shift /
    scale: n = (x - mu) / sigma, nd = (xd - mean(xd) - n mean(n xd)) / sigma; y = n (1 + s) + b, yd = nd (1 + s) + n sd + bd.
    drop_mod_tangent: without the n sd + bd terms."""
    mu = x.mean(-1, keepdim=True)
    sigma = torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-6)
    n = (x - mu) / sigma
    nd = (xd - xd.mean(-1, keepdim=True) - n * (n * xd).mean(-1, keepdim=True)) / sigma
    y = n * (1 + scale.unsqueeze(1)) + shift.unsqueeze(1)
    yd = nd * (1 + scale.unsqueeze(1))
    if not drop_mod_tangent:
        yd = yd + n * scaled.unsqueeze(1) + shiftd.unsqueeze(1)
    return y, yd


def attention_core_jvp(q: Tensor, k: Tensor, v: Tensor, qd: Tensor, kd: Tensor, vd: Tensor, drop_softmax_term: bool = False):
    """softmax(q k^T / sqrt(hd)) v of the restated timm Attention (oracle/dit_ref.py `attention`) on [B, H, N, hd] with tangent:
    Sd = (qd k^T + q kd^T) / sqrt(hd), delta_i = sum_j P_ij Sd_ij, Od = (P o (Sd - delta)) v + P vd.
    drop_softmax_term: Od = P vd only."""
    sc = q.shape[-1] ** -0.5
    p = ((q * sc) @ k.transpose(-2, -1)).softmax(dim=-1)
    o = p @ v
    od = p @ vd
    if not drop_softmax_term:
        sdot = (qd @ k.transpose(-2, -1) + q @ kd.transpose(-2, -1)) * sc
        delta = (p * sdot).sum(-1, keepdim=True)
        od = od + (p * (sdot - delta)) @ v
    return o, od


def attention_jvp(sd, b: str, x: Tensor, xd: Tensor, heads: int, drop_softmax_term: bool = False):
    """oracle `attention` (qkv Linear, head split, core, proj Linear) with tangent; also returns the un-projected core outputs."""
    B, N, D = x.shape
    hd = D // heads
    wq, bq, wp, bp = (sd[b + k] for k in ("attention.qkv.weight", "attention.qkv.bias", "attention.proj.weight", "attention.proj.bias"))
    split = lambda a: a.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)  # noqa: E731
    q, k, v = split(F.linear(x, wq, bq))
    qd, kd, vd = split(F.linear(xd, wq))
    o, od = attention_core_jvp(q, k, v, qd, kd, vd, drop_softmax_term)
    o, od = o.transpose(1, 2).reshape(B, N, D), od.transpose(1, 2).reshape(B, N, D)
    return F.linear(o, wp, bp), F.linear(od, wp)


def gelu_jvp(h: Tensor, hd: Tensor):
    """GELU(approximate="tanh") (:176) = h sig(2 u), u = sqrt(2 / pi) (h + 0.044715 h^3); derivative sig + h sig (1 - sig) 2 u'."""
    c0, c1 = math.sqrt(2.0 / math.pi), 0.044715
    sig = torch.sigmoid(2 * c0 * h * (1 + c1 * h * h))
    g = h * sig
    return g, (sig + g * (1 - sig) * 2 * c0 * (1 + 3 * c1 * h * h)) * hd


def dit_block_jvp(sd, i: int, x: Tensor, xd: Tensor, c: Tensor, cd: Tensor, heads: int, drop_softmax_term: bool = False,
                  drop_gate_tangent: bool = False, drop_mod_tangent: bool = False):
    """DiTBlock.forward, :184-201, with tangent: modd = W_mod (silu'(c) o cd); x' = x + g o h, xd' = xd + g o hd + gd o h.
    drop_gate_tangent: without the gd o h terms."""
    b = f"blocks.{i}."
    s, sdd = silu_jvp(c, cd)
    wm = sd[b + "conditioning_net.1.weight"]
    a_shift, a_scale, a_gate, f_shift, f_scale, f_gate = F.linear(s, wm, sd[b + "conditioning_net.1.bias"]).chunk(6, dim=1)
    a_shiftd, a_scaled, a_gated, f_shiftd, f_scaled, f_gated = F.linear(sdd, wm).chunk(6, dim=1)
    y, yd = ln_modulate_jvp(x, xd, a_shift, a_shiftd, a_scale, a_scaled, drop_mod_tangent)
    h, hd = attention_jvp(sd, b, y, yd, heads, drop_softmax_term)
    xd = xd + a_gate.unsqueeze(1) * hd + (0 if drop_gate_tangent else a_gated.unsqueeze(1) * h)
    x = x + a_gate.unsqueeze(1) * h
    y, yd = ln_modulate_jvp(x, xd, f_shift, f_shiftd, f_scale, f_scaled, drop_mod_tangent)
    w1, b1, w2, b2 = (sd[b + k] for k in ("feed_forward.fc1.weight", "feed_forward.fc1.bias", "feed_forward.fc2.weight", "feed_forward.fc2.bias"))
    a, ad = gelu_jvp(F.linear(y, w1, b1), F.linear(yd, w1))
    h, hd = F.linear(a, w2, b2), F.linear(ad, w2)
    xd = xd + f_gate.unsqueeze(1) * hd + (0 if drop_gate_tangent else f_gated.unsqueeze(1) * h)
    x = x + f_gate.unsqueeze(1) * h
    return x, xd


def final_layer_jvp(sd, cfg, x: Tensor, xd: Tensor, c: Tensor, cd: Tensor, drop_mod_tangent: bool = False):
    """OutputProjection (:204-225) + unpatchify (:437-455) of both streams."""
    B, p, C = x.shape[0], cfg.patch_size, cfg.in_channels
    s, sdd = silu_jvp(c, cd)
    wm = sd["final_layer.adaptive_params.1.weight"]
    shift, scale = F.linear(s, wm, sd["final_layer.adaptive_params.1.bias"]).chunk(2, dim=1)
    shiftd, scaled = F.linear(sdd, wm).chunk(2, dim=1)
    y, yd = ln_modulate_jvp(x, xd, shift, shiftd, scale, scaled, drop_mod_tangent)
    w = sd["final_layer.projection.weight"]
    g = math.isqrt(x.shape[1])
    unp = lambda a: torch.einsum("bhwpqc->bchpwq", a.reshape(B, g, g, p, p, C)).reshape(B, C, g * p, g * p)  # noqa: E731
    return unp(F.linear(y, w, sd["final_layer.projection.bias"])), unp(F.linear(yd, w))


def dit_jvp_raw(sd, cfg, x_t: Tensor, t_e: Tensor, r_e: Optional[Tensor], cls: Tensor, vx: Tensor, vt_e: Tensor, vr_e: Optional[Tensor], **drop):
    """What fg_dit_jvp computes: the raw network output and its tangent, t_e / r_e / vt_e / vr_e as the embedders see them."""
    w = sd["x_embedder.proj.weight"]
    x = F.conv2d(x_t, w, sd["x_embedder.proj.bias"], stride=cfg.patch_size).flatten(2).transpose(1, 2) + sd["pos_embed"]
    xd = F.conv2d(vx, w, None, stride=cfg.patch_size).flatten(2).transpose(1, 2)  # linear: no bias, no pos_embed (:270, 511)
    c, cd = time_embedding_jvp(sd, "t_embedder", t_e, vt_e)
    c = c + sd["y_embedder.class_embeddings.weight"][cls]
    if cfg.r_timestep and r_e is not None:
        e, ed = time_embedding_jvp(sd, "r_embedder", r_e, vr_e)
        c, cd = c + e, cd + ed
    blk = {k: v for k, v in drop.items() if k != "flip_vr"}
    for i in range(cfg.depth):
        x, xd = dit_block_jvp(sd, i, x, xd, c, cd, cfg.num_heads, **blk)
    return final_layer_jvp(sd, cfg, x, xd, c, cd, blk.get("drop_mod_tangent", False))


def dit_jvp(sd, cfg, x_t: Tensor, t: Tensor, cls: Tensor, r: Optional[Tensor], vx: Tensor, vt: Tensor, vr: Optional[Tensor], **drop):
    """(output, tangent) of oracle `dit_forward(sd, cfg, x_t, t, cls, r)` along (vx, vt, vr): its preparation of (t, r) (:457-462,
    503-504, 520-521) and the chain rule of that preparation - x 1000 under scale_t, the sign under the SiT convention, vt - vr under
    time_cond_type 'diff' - around dit_jvp_raw; both results negated under the SiT convention (:555-558).
    flip_vr: the 'diff' rule with the wrong sign of vr."""
    k = 1000.0 if cfg.scale_t else 1.0
    t_e, vt_e = k * t, k * vt
    use_r = cfg.r_timestep and r is not None
    r_e, vr_e = (k * r, k * vr) if use_r else (None, None)
    if cfg.use_sit_convention:
        t_e, vt_e = 1 - t_e, -vt_e
    if use_r and cfg.time_cond_type == "diff":
        r_e, vr_e = t_e - r_e, (vt_e + vr_e if drop.get("flip_vr") else vt_e - vr_e)
    out, jv = dit_jvp_raw(sd, cfg, x_t, t_e, r_e, cls, vx, vt_e, vr_e, **drop)
    return (-out, -jv) if cfg.use_sit_convention else (out, jv)


def oracle_jvp(sd, cfg, x_t: Tensor, t: Tensor, cls: Tensor, r: Optional[Tensor], vx: Tensor, vt: Tensor, vr: Optional[Tensor]):
    """The reference of the GPU tests: torch.func.jvp over the oracle's own dit_forward (what MeanFlowModel._jvp evaluates, mean_flow.py:240-250)."""
    if r is None:
        return torch.func.jvp(lambda a, b: R.dit_forward(sd, cfg, a, b, cls), (x_t, t), (vx, vt))
    return torch.func.jvp(lambda a, b, c: R.dit_forward(sd, cfg, a, b, cls, c), (x_t, t, r), (vx, vt, vr))
