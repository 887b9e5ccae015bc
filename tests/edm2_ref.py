"""Functional fp32 restatement of the EDM2 U-Net and its preconditioning (EDM2Precond / EMD2UNet / Block of the reference's
fastgen/networks/EDM2/network.py) over flat state dicts, written from the EDM2 paper's equations: the magnitude-preserving
conv (eq. 47), pixel norm, mp_silu (eq. 81), mp_sum (eq. 88), mp_cat (eq. 103), MP-Fourier features (eq. 75) and the
cosine attention.  Pinned to reference-recorded fixtures by tests/test_edm2.py; the GPU tests compare against it."""
import math
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor


@dataclass
class EDM2Config:
    img_resolution: int = 64
    img_channels: int = 3
    label_dim: int = 1000
    model_channels: int = 192
    channel_mult: List[int] = field(default_factory=lambda: [1, 2, 3, 4])
    num_blocks: int = 3
    attn_resolutions: List[int] = field(default_factory=lambda: [16, 8])
    label_balance: float = 0.5
    concat_balance: float = 0.5
    res_balance: float = 0.3
    attn_balance: float = 0.3
    clip_act: Optional[float] = 256
    logvar_channels: int = 128
    sigma_data: float = 0.5

    def kwargs(self) -> dict:
        return dict(img_resolution=self.img_resolution, img_channels=self.img_channels, label_dim=self.label_dim,
                    model_channels=self.model_channels, channel_mult=list(self.channel_mult), num_blocks=self.num_blocks,
                    attn_resolutions=list(self.attn_resolutions), label_balance=self.label_balance,
                    concat_balance=self.concat_balance, res_balance=self.res_balance, attn_balance=self.attn_balance,
                    clip_act=self.clip_act, logvar_channels=self.logvar_channels, sigma_data=self.sigma_data)


IN64_S = EDM2Config()
NARROW = EDM2Config(model_channels=64, num_blocks=1, label_dim=10)
SMALL_UNCOND = EDM2Config(img_resolution=16, model_channels=64, channel_mult=[1, 2], num_blocks=1, attn_resolutions=[8],
                          label_dim=0)


@dataclass
class Blk:
    key: str
    enc: bool
    cin: int
    cout: int
    res_in: int
    res_out: int
    up: bool = False
    down: bool = False
    attn: bool = False
    skip_c: int = 0


def layout(cfg: EDM2Config):
    """(encoder blocks, decoder blocks, stem width, out_conv input width, encoder output widths) in module order."""
    widths = [cfg.model_channels * m for m in cfg.channel_mult]
    enc: List[Blk] = []
    dec: List[Blk] = []
    skips: List[int] = []
    c = widths[0]
    for lvl, w in enumerate(widths):
        r = cfg.img_resolution >> lvl
        if lvl > 0:
            enc.append(Blk(f"unet.enc.{r}x{r}_down", True, c, c, 2 * r, r, down=True))
        skips.append(c)
        for i in range(cfg.num_blocks):
            enc.append(Blk(f"unet.enc.{r}x{r}_block{i}", True, c, w, r, r, attn=r in cfg.attn_resolutions))
            c = w
            skips.append(c)
    enc_out = list(skips)
    for lvl in reversed(range(len(widths))):
        r = cfg.img_resolution >> lvl
        if lvl == len(widths) - 1:
            dec.append(Blk(f"unet.dec.{r}x{r}_in0", False, c, c, r, r, attn=True))
            dec.append(Blk(f"unet.dec.{r}x{r}_in1", False, c, c, r, r))
        else:
            dec.append(Blk(f"unet.dec.{r}x{r}_up", False, c, c, r // 2, r, up=True))
        for i in range(cfg.num_blocks + 1):
            s = skips.pop()
            dec.append(Blk(f"unet.dec.{r}x{r}_block{i}", False, c + s, widths[lvl], r, r, attn=r in cfg.attn_resolutions, skip_c=s))
            c = widths[lvl]
    return enc, dec, widths[0], c, enc_out


def state_shapes(cfg: EDM2Config) -> "OrderedDict[str, tuple]":
    enc, dec, stem, out_cin, _ = layout(cfg)
    cnoise, cemb = cfg.model_channels * cfg.channel_mult[0], cfg.model_channels * max(cfg.channel_mult)
    d = OrderedDict()
    d["unet.out_gain"] = (1,)
    d["unet.emb_fourier.freqs"] = (cnoise,)
    d["unet.emb_fourier.phases"] = (cnoise,)
    d["unet.emb_noise.weight"] = (cemb, cnoise)
    if cfg.label_dim:
        d["unet.emb_label.weight"] = (cemb, cfg.label_dim)
    r = cfg.img_resolution

    def block(b: Blk):
        p = b.key + "."
        d[p + "emb_gain"] = (1,)
        d[p + "conv_res0.weight"] = (b.cout, b.cout if b.enc else b.cin, 3, 3)
        d[p + "emb_linear.weight"] = (b.cout, cemb)
        d[p + "conv_res1.weight"] = (b.cout, b.cout, 3, 3)
        if b.cin != b.cout:
            d[p + "conv_skip.weight"] = (b.cout, b.cin, 1, 1)
        if b.attn:
            d[p + "attn_qkv.weight"] = (3 * b.cout, b.cout, 1, 1)
            d[p + "attn_proj.weight"] = (b.cout, b.cout, 1, 1)

    d[f"unet.enc.{r}x{r}_conv.weight"] = (stem, cfg.img_channels + 1, 3, 3)
    for b in enc:
        block(b)
    for b in dec:
        block(b)
    d["unet.out_conv.weight"] = (cfg.img_channels, out_cin, 3, 3)
    d["logvar_fourier.freqs"] = (cfg.logvar_channels,)
    d["logvar_fourier.phases"] = (cfg.logvar_channels,)
    d["logvar_linear.weight"] = (1, cfg.logvar_channels)
    return d


def random_state_dict(cfg: EDM2Config, seed: int = 1234) -> Dict[str, Tensor]:
    """Seeded weights.  The reference initialises every emb_gain and out_gain to zero (the output is then exactly zero and every
    modulation exactly one); here they are random: emb_gain ~ 0.3 + 0.1 N(0, 1), out_gain ~ 0.6 + 0.1 N(0, 1).  Conv / linear
    weights ~ N(0, 1) (MPConv normalises them), Fourier buffers as MPFourier draws them."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, Tensor] = {}
    for name, shape in state_shapes(cfg).items():
        if name.endswith("freqs"):
            sd[name] = 2 * np.pi * torch.randn(shape, generator=g)
        elif name.endswith("phases"):
            sd[name] = 2 * np.pi * torch.rand(shape, generator=g)
        elif name.endswith("emb_gain"):
            sd[name] = 0.3 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith("out_gain"):
            sd[name] = 0.6 + 0.1 * torch.randn(shape, generator=g)
        else:
            sd[name] = torch.randn(shape, generator=g)
    return sd


def subsample(v: Tensor, stride: int = 61) -> Tensor:
    return v.reshape(-1)[::stride].clone()


# ---- layers ------------------------------------------------------------------------------------------------------------------
def unit_rows(w: Tensor) -> Tensor:
    """w / (1e-4 + |w_o| / sqrt(fan_in)) per output row."""
    fan = w[0].numel()
    n = torch.linalg.vector_norm(w.reshape(w.shape[0], -1), dim=1).reshape(-1, *([1] * (w.ndim - 1)))
    return w / (1e-4 + n / math.sqrt(fan))


def mp_weight(w: Tensor, gain=1.0) -> Tensor:
    return unit_rows(w) * (gain / math.sqrt(w[0].numel()))


def mp_linear(x: Tensor, w: Tensor, gain=1.0) -> Tensor:
    return x @ mp_weight(w.to(x.dtype), gain).t()


def mp_conv(x: Tensor, w: Tensor, gain=1.0) -> Tensor:
    return F.conv2d(x, mp_weight(w.to(x.dtype), gain), padding=w.shape[-1] // 2)


def pixel_norm(x: Tensor, dim: int = 1) -> Tensor:
    n = torch.linalg.vector_norm(x, dim=dim, keepdim=True)
    return x / (1e-4 + n / math.sqrt(x.shape[dim]))


def mp_silu(x: Tensor) -> Tensor:
    return F.silu(x) / 0.596


def mp_sum(a: Tensor, b: Tensor, t: float) -> Tensor:
    return ((1 - t) * a + t * b) / math.sqrt((1 - t) ** 2 + t ** 2)


def mp_cat(a: Tensor, b: Tensor, t: float) -> Tensor:
    na, nb = a.shape[1], b.shape[1]
    c = math.sqrt((na + nb) / ((1 - t) ** 2 + t ** 2))
    return torch.cat([a * (c / math.sqrt(na) * (1 - t)), b * (c / math.sqrt(nb) * t)], dim=1)


def fourier(x: Tensor, freqs: Tensor, phases: Tensor) -> Tensor:
    return torch.cos(x[:, None] * freqs[None].to(x.dtype) + phases[None].to(x.dtype)) * math.sqrt(2)


def block(sd, b: Blk, cfg: EDM2Config, x: Tensor, emb: Tensor) -> Tensor:
    p = b.key + "."
    if b.down:
        x = F.avg_pool2d(x, 2)
    elif b.up:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    if b.enc:
        if p + "conv_skip.weight" in sd:
            x = mp_conv(x, sd[p + "conv_skip.weight"])
        x = pixel_norm(x)
    y = mp_conv(mp_silu(x), sd[p + "conv_res0.weight"])
    c = mp_linear(emb, sd[p + "emb_linear.weight"], gain=sd[p + "emb_gain"].to(emb.dtype)) + 1
    y = mp_conv(mp_silu(y * c[:, :, None, None]), sd[p + "conv_res1.weight"])
    if not b.enc and p + "conv_skip.weight" in sd:
        x = mp_conv(x, sd[p + "conv_skip.weight"])
    x = mp_sum(x, y, cfg.res_balance)
    if b.attn:
        B, C, H, W = x.shape
        heads = C // 64
        qkv = mp_conv(x, sd[p + "attn_qkv.weight"]).reshape(B, heads, 64, 3, H * W)
        qkv = pixel_norm(qkv, dim=2)
        q, k, v = qkv.unbind(3)
        a = torch.softmax(torch.einsum("bhcq,bhck->bhqk", q, k) / 8, dim=3)
        y = torch.einsum("bhqk,bhck->bhcq", a, v).reshape(B, C, H, W)
        x = mp_sum(x, mp_conv(y, sd[p + "attn_proj.weight"]), cfg.attn_balance)
    if cfg.clip_act is not None:
        x = x.clamp(-cfg.clip_act, cfg.clip_act)
    return x


def embedding(sd, cfg: EDM2Config, c_noise: Tensor, labels: Optional[Tensor]) -> Tensor:
    emb = mp_linear(fourier(c_noise, sd["unet.emb_fourier.freqs"], sd["unet.emb_fourier.phases"]), sd["unet.emb_noise.weight"])
    if cfg.label_dim:
        if labels is None:
            labels = torch.zeros(1, cfg.label_dim, dtype=emb.dtype)
        emb = mp_sum(emb, mp_linear(labels * math.sqrt(cfg.label_dim), sd["unet.emb_label.weight"]), cfg.label_balance)
    return mp_silu(emb)


def unet(sd, cfg: EDM2Config, x: Tensor, c_noise: Tensor, labels: Optional[Tensor], trace: Optional[dict] = None) -> Tensor:
    enc, dec, _, _, _ = layout(cfg)
    emb = embedding(sd, cfg, c_noise, labels)
    if trace is not None:
        trace["emb"] = emb
    r = cfg.img_resolution
    x = mp_conv(torch.cat([x, torch.ones_like(x[:, :1])], 1), sd[f"unet.enc.{r}x{r}_conv.weight"])
    skips = [x]
    if trace is not None:
        trace["stem"] = x
    for b in enc:
        x = block(sd, b, cfg, x, emb)
        skips.append(x)
        if trace is not None:
            trace[b.key] = x
    for b in dec:
        if b.skip_c:
            x = mp_cat(x, skips.pop(), cfg.concat_balance)
        x = block(sd, b, cfg, x, emb)
        if trace is not None:
            trace[b.key] = x
    x = mp_conv(x, sd["unet.out_conv.weight"], gain=sd["unet.out_gain"].to(x.dtype))
    if trace is not None:
        trace["F"] = x
    return x


def precond_forward(sd, cfg: EDM2Config, x_t: Tensor, t: Tensor, condition: Optional[Tensor], sigma_shift: float = 0.0,
                    trace: Optional[dict] = None, drop_precond: Optional[str] = None) -> Tensor:
    """EDM2Precond.forward in eval mode, x0 prediction; t float64 [B].  drop_precond None / "input" / "output" / "both": "input" skips
    precond_input (the U-Net sees x_t and t as they are), "output" skips precond_output (the result is the U-Net's own output)."""
    assert drop_precond in (None, "input", "output", "both")
    t = t.to(torch.float64)
    sd2 = cfg.sigma_data ** 2
    if drop_precond in ("input", "both"):
        F_x = unet(sd, cfg, x_t, t.to(x_t.dtype), condition, trace)
    else:
        c_in = (1 / (sd2 + t ** 2).sqrt()).to(x_t.dtype)
        c_noise = (t.clamp(min=1e-6).log() / 4).to(x_t.dtype)
        F_x = unet(sd, cfg, x_t * c_in[:, None, None, None], c_noise, condition, trace)
    if drop_precond in ("output", "both"):
        return F_x
    ts = t - sigma_shift
    c_skip = (sd2 / (ts ** 2 + sd2)).to(x_t.dtype)
    c_out = (ts * cfg.sigma_data / (ts ** 2 + sd2).sqrt()).to(x_t.dtype)
    return c_skip[:, None, None, None] * x_t + c_out[:, None, None, None] * F_x


def logvar(sd, t: Tensor) -> Tensor:
    c_noise = (t.to(torch.float64).clamp(min=1e-6).log() / 4).to(torch.float32)
    return mp_linear(fourier(c_noise, sd["logvar_fourier.freqs"], sd["logvar_fourier.phases"]), sd["logvar_linear.weight"]).reshape(-1, 1)
