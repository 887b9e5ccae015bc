"""Functional CPU restatement of EDMPrecond(model_type="DhariwalUNet") (reference fastgen/networks/EDM/network.py:584-740,
UNetBlock :205-303, EDMPrecond.forward :881-974), built on oracle/edm_ref.py's layers.  fp32 torch ops in the reference's order;
tests/test_dhariwal.py pins it to the fixture recorded from the reference itself (scripts/gen_golden_dhariwal.py), and the GPU
tests compare the HIP path against it."""
from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

from oracle.edm_ref import attention as attention_fp32
from oracle.edm_ref import conv2d, edm_t_list, forward_process, group_norm, latents, linear, x0_to_eps

EPS = 1e-5  # GroupNorm / UNetBlock eps of DhariwalUNet (EDM/network.py:134, 218)


@dataclass
class DhariwalConfig:
    img_resolution: int = 64
    img_channels: int = 3
    label_dim: int = 1000
    augment_dim: int = 0
    model_channels: int = 192
    channel_mult: Tuple[int, ...] = (1, 2, 3, 4)
    channel_mult_emb: int = 4
    num_blocks: int = 3
    attn_resolutions: Tuple[int, ...] = (32, 16, 8)
    sigma_data: float = 0.5
    sigma_shift: float = 0.0

    def kwargs(self) -> dict:
        """EDMPrecond constructor kwargs of this config (EDM_ImageNet64_Config, fastgen/configs/net.py:50-66, for IN64)."""
        return dict(img_resolution=self.img_resolution, img_channels=self.img_channels, label_dim=self.label_dim,
                    sigma_shift=self.sigma_shift, sigma_data=self.sigma_data, model_type="DhariwalUNet", augment_dim=self.augment_dim,
                    model_channels=self.model_channels, channel_mult=list(self.channel_mult), channel_mult_emb=self.channel_mult_emb,
                    num_blocks=self.num_blocks, attn_resolutions=list(self.attn_resolutions), dropout=0.0, label_dropout=0,
                    r_timestep=False, drop_precond=None)


IN64 = DhariwalConfig()
# fixture (a): every block kind and GroupNorm group-size class at full resolution, narrow
NARROW = DhariwalConfig(model_channels=64, num_blocks=1, label_dim=10, augment_dim=9)


@dataclass
class Block:
    key: str
    cin: int
    cout: int
    res: int  # output resolution
    up: bool = False
    down: bool = False
    attn: bool = False


def layout(cfg: DhariwalConfig):
    """(stem channels, encoder blocks, decoder blocks) in module order (EDM/network.py:656-691)."""
    enc: List[Block] = []
    dec: List[Block] = []
    cout = cfg.img_channels
    skips = []
    stem = None
    for level, mult in enumerate(cfg.channel_mult):
        res = cfg.img_resolution >> level
        if level == 0:
            stem = cfg.model_channels * mult
            cout = stem
        else:
            enc.append(Block(f"{res}x{res}_down", cout, cout, res, down=True))
        skips.append(cout)
        for idx in range(cfg.num_blocks):
            cin, cout = cout, cfg.model_channels * mult
            enc.append(Block(f"{res}x{res}_block{idx}", cin, cout, res, attn=res in cfg.attn_resolutions))
            skips.append(cout)
    for level, mult in reversed(list(enumerate(cfg.channel_mult))):
        res = cfg.img_resolution >> level
        if level == len(cfg.channel_mult) - 1:
            dec.append(Block(f"{res}x{res}_in0", cout, cout, res, attn=True))
            dec.append(Block(f"{res}x{res}_in1", cout, cout, res))
        else:
            dec.append(Block(f"{res}x{res}_up", cout, cout, res, up=True))
        for idx in range(cfg.num_blocks + 1):
            cin, cout = cout + skips.pop(), cfg.model_channels * mult
            dec.append(Block(f"{res}x{res}_block{idx}", cin, cout, res, attn=res in cfg.attn_resolutions))
    return stem, enc, dec


def state_shapes(cfg: DhariwalConfig) -> "OrderedDict[str, tuple]":
    """Every state_dict() entry (parameters and the resample_filter buffers) of the reference module, in its order."""
    E, N = cfg.model_channels * cfg.channel_mult_emb, cfg.model_channels
    s: "OrderedDict[str, tuple]" = OrderedDict()
    if cfg.augment_dim:
        s["model.map_augment.weight"] = (N, cfg.augment_dim)
    s["model.map_layer0.weight"], s["model.map_layer0.bias"] = (E, N), (E,)
    s["model.map_layer1.weight"], s["model.map_layer1.bias"] = (E, E), (E,)
    if cfg.label_dim:
        s["model.map_label.weight"] = (E, cfg.label_dim)
    stem, enc, dec = layout(cfg)
    R = cfg.img_resolution
    s[f"model.enc.{R}x{R}_conv.weight"], s[f"model.enc.{R}x{R}_conv.bias"] = (stem, cfg.img_channels, 3, 3), (stem,)

    def block(prefix, b: Block):
        p = f"{prefix}.{b.key}."
        s[p + "norm0.weight"], s[p + "norm0.bias"] = (b.cin,), (b.cin,)
        s[p + "conv0.weight"], s[p + "conv0.bias"] = (b.cout, b.cin, 3, 3), (b.cout,)
        if b.up or b.down:
            s[p + "conv0.resample_filter"] = (1, 1, 2, 2)
        s[p + "affine.weight"], s[p + "affine.bias"] = (2 * b.cout, E), (2 * b.cout,)
        s[p + "norm1.weight"], s[p + "norm1.bias"] = (b.cout,), (b.cout,)
        s[p + "conv1.weight"], s[p + "conv1.bias"] = (b.cout, b.cout, 3, 3), (b.cout,)
        if b.cin != b.cout:
            s[p + "skip.weight"], s[p + "skip.bias"] = (b.cout, b.cin, 1, 1), (b.cout,)
        elif b.up or b.down:
            s[p + "skip.resample_filter"] = (1, 1, 2, 2)
        if b.attn:
            s[p + "norm2.weight"], s[p + "norm2.bias"] = (b.cout,), (b.cout,)
            s[p + "qkv.weight"], s[p + "qkv.bias"] = (3 * b.cout, b.cout, 1, 1), (3 * b.cout,)
            s[p + "proj.weight"], s[p + "proj.bias"] = (b.cout, b.cout, 1, 1), (b.cout,)

    for b in enc:
        block("model.enc", b)
    for b in dec:
        block("model.dec", b)
    C = dec[-1].cout
    s["model.out_norm.weight"], s["model.out_norm.bias"] = (C,), (C,)
    s["model.out_conv.weight"], s["model.out_conv.bias"] = (cfg.img_channels, C, 3, 3), (cfg.img_channels,)
    s["model.logvar_linear.weight"], s["model.logvar_linear.bias"] = (1, cfg.model_channels), (1,)
    return s


def subsample(v: Tensor, stride: int = 61) -> Tensor:
    """Every stride-th element of the flattened tensor (the recorded form of large fixture tensors)."""
    return v.reshape(-1)[::stride].clone()


def random_state_dict(cfg: DhariwalConfig, seed: int = 1234) -> Dict[str, Tensor]:
    """Seeded weights that keep every branch O(1) (the reference init zeroes conv1 / proj / out_conv, which would make the
    output trivial): matrices ~ N(0, 1/fan_in), norm gains ~ 1 + 0.1 N(0,1), biases ~ 0.1 N(0,1); affine weights at a tenth
    (scale + 1 stays near 1); the constant resample filters at 0.25."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, Tensor] = {}
    for name, shape in state_shapes(cfg).items():
        if name.endswith("resample_filter"):
            sd[name] = torch.full(shape, 0.25)
        elif len(shape) == 1:
            base = 1.0 if "norm" in name and name.endswith("weight") else 0.0
            sd[name] = base + 0.1 * torch.randn(shape, generator=g)
        else:
            w = torch.randn(shape, generator=g) / math.sqrt(int(np.prod(shape[1:])))
            sd[name] = w * 0.1 if ".affine." in name else w
    return sd


def positional_embedding(t: Tensor, num_channels: int, max_positions: int = 10000) -> Tensor:
    """PositionalEmbedding(endpoint=False).forward, EDM/network.py:306-319 -> [cos | sin] (DhariwalUNet does not flip it)."""
    half = num_channels // 2
    freqs = torch.arange(0, half, dtype=torch.float32) / half
    freqs = (1 / max_positions) ** freqs
    ang = t.ger(freqs.to(device=t.device, dtype=t.dtype))
    return torch.cat([ang.cos(), ang.sin()], dim=1)


def mapping(sd, cfg: DhariwalConfig, noise_labels: Tensor, class_labels: Optional[Tensor], augment_labels=None) -> Tensor:
    """DhariwalUNet.forward mapping part (EDM/network.py:705-726)."""
    emb = positional_embedding(noise_labels, cfg.model_channels)
    if augment_labels is not None and "model.map_augment.weight" in sd:
        emb = emb + linear(augment_labels, sd["model.map_augment.weight"], None)
    emb = F.silu(linear(emb, sd["model.map_layer0.weight"], sd["model.map_layer0.bias"]))
    emb = linear(emb, sd["model.map_layer1.weight"], sd["model.map_layer1.bias"])
    if cfg.label_dim:
        emb = emb + linear(class_labels, sd["model.map_label.weight"], None)
    return F.silu(emb)


def resample(x: Tensor, up: bool, down: bool) -> Tensor:
    """The weightless part of Conv2d.forward with resample_filter=[1, 1] (EDM/network.py:113-121), as oracle.edm_ref.conv2d does it,
    on x's device."""
    c = x.shape[1]
    if up:
        x = F.conv_transpose2d(x, torch.ones(c, 1, 2, 2, dtype=x.dtype, device=x.device), groups=c, stride=2)
    if down:
        x = F.conv2d(x, torch.full((c, 1, 2, 2), 0.25, dtype=x.dtype, device=x.device), groups=c, stride=2)
    return x


def conv(x: Tensor, w: Optional[Tensor], b: Optional[Tensor], up=False, down=False) -> Tensor:
    return conv2d(resample(x, up, down), w, b)


def attention(qkv: Tensor, heads: int) -> Tensor:
    """oracle.edm_ref.attention (logits and softmax in fp32, as the reference runs them); an fp64 qkv stays fp64 throughout, so that
    the fp64 references of the kernel-parity tests carry no fp32 rounding."""
    if qkv.dtype != torch.float64:
        return attention_fp32(qkv, heads)
    B, C3, H, W = qkv.shape
    C = C3 // 3
    q, k, v = qkv.reshape(B * heads, C // heads, 3, H * W).unbind(2)
    w = torch.einsum("ncq,nck->nqk", q, k / math.sqrt(k.shape[1])).softmax(dim=2)
    return torch.einsum("nqk,nck->ncq", w, v).reshape(B, C, H, W)


def unet_block(sd, prefix: str, b: Block, x: Tensor, emb: Tensor) -> Tensor:
    """UNetBlock.forward with adaptive_scale=True, skip_scale=1, num_heads = cout / 64 (EDM/network.py:274-299)."""
    p = f"{prefix}.{b.key}."
    orig = x
    x = conv(F.silu(group_norm(x, sd[p + "norm0.weight"], sd[p + "norm0.bias"], EPS)), sd[p + "conv0.weight"], sd[p + "conv0.bias"],
             up=b.up, down=b.down)
    params = linear(emb, sd[p + "affine.weight"], sd[p + "affine.bias"]).unsqueeze(2).unsqueeze(3)
    scale, shift = params.chunk(chunks=2, dim=1)
    x = F.silu(torch.addcmul(shift, group_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], EPS), scale + 1))
    x = conv2d(x, sd[p + "conv1.weight"], sd[p + "conv1.bias"])
    if b.cin != b.cout:
        x = x + conv2d(orig, sd[p + "skip.weight"], sd[p + "skip.bias"])
    elif b.up or b.down:
        x = x + resample(orig, b.up, b.down)
    else:
        x = x + orig
    if b.attn:
        qkv = conv2d(group_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], EPS), sd[p + "qkv.weight"], sd[p + "qkv.bias"])
        x = conv2d(attention(qkv, b.cout // 64), sd[p + "proj.weight"], sd[p + "proj.bias"]) + x
    return x


def dhariwal_unet(sd, cfg: DhariwalConfig, x: Tensor, noise_labels: Tensor, class_labels, trace: Optional[dict] = None,
                  augment_labels=None) -> Tensor:
    """DhariwalUNet.forward (EDM/network.py:693-740) without feature taps.  trace (optional): 'emb' and every block output."""
    emb = mapping(sd, cfg, noise_labels, class_labels, augment_labels)
    if trace is not None:
        trace["emb"] = emb
    stem, enc, dec = layout(cfg)
    R = cfg.img_resolution
    x = conv2d(x, sd[f"model.enc.{R}x{R}_conv.weight"], sd[f"model.enc.{R}x{R}_conv.bias"])
    skips = [x]
    for b in enc:
        x = unet_block(sd, "model.enc", b, x, emb)
        if trace is not None:
            trace[f"enc.{b.key}"] = x
        skips.append(x)
    for b in dec:
        if x.shape[1] != b.cin:
            x = torch.cat([x, skips.pop()], dim=1)
        x = unet_block(sd, "model.dec", b, x, emb)
        if trace is not None:
            trace[f"dec.{b.key}"] = x
    x = F.silu(group_norm(x, sd["model.out_norm.weight"], sd["model.out_norm.bias"], EPS))
    return conv2d(x, sd["model.out_conv.weight"], sd["model.out_conv.bias"])


def precond_forward(sd, cfg: DhariwalConfig, x_t: Tensor, t: Tensor, condition: Optional[Tensor], trace=None,
                    augment_labels=None) -> Tensor:
    """EDMPrecond.forward, eval mode, fwd_pred_type = 'x0' (EDM/network.py:881-974; precond_input / precond_output :755-805)."""
    B = x_t.shape[0]
    t = t.to(torch.float64).reshape(-1)
    if cfg.label_dim == 0:
        class_labels = None
    elif condition is None:
        class_labels = torch.zeros(1, cfg.label_dim, dtype=x_t.dtype)
    else:
        class_labels = condition.reshape(-1, cfg.label_dim)
    c_in = (1.0 / (cfg.sigma_data**2 + t**2).sqrt()).to(x_t.dtype).reshape(B, 1, 1, 1)
    t_in = (t.clamp(min=1e-6).log() / 4).to(x_t.dtype)
    F_x = dhariwal_unet(sd, cfg, c_in * x_t, t_in, class_labels, trace=trace, augment_labels=augment_labels)
    ts = t - cfg.sigma_shift
    c_skip = (cfg.sigma_data**2 / (ts**2 + cfg.sigma_data**2)).to(x_t.dtype).reshape(B, 1, 1, 1)
    c_out = (ts * cfg.sigma_data / (ts**2 + cfg.sigma_data**2).sqrt()).to(x_t.dtype).reshape(B, 1, 1, 1)
    return c_skip * x_t + c_out * F_x


def generator_fn(sd, cfg: DhariwalConfig, noise: Tensor, condition, steps: int, sample_type: str = "sde", eps_list=None,
                 t_list=None) -> Tensor:
    """FastGenModel.generator_fn + _student_sample_loop (methods/model.py:315-420) with the 'sde' noise injected via eps_list."""
    with torch.inference_mode():
        t_list = edm_t_list(steps) if t_list is None else torch.as_tensor(t_list, dtype=torch.float64)
        B = noise.shape[0]
        x = latents(noise, t_list[0])
        x_pred = x
        for i, (t_cur, t_next) in enumerate(zip(t_list[:-1], t_list[1:])):
            x_pred = precond_forward(sd, cfg, x, t_cur.expand(B), condition)
            if t_next > 0:
                eps = eps_list[i] if sample_type == "sde" else x0_to_eps(x, x_pred, t_cur.expand(B))
                x = forward_process(x_pred, eps, t_next.expand(B))
        return x_pred
