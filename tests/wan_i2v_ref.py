"""The image-to-video network (reference fastgen/networks/WanI2V/network.py `WanI2V`, Wan2.1-I2V convention: concat_mask = True,
use_image_encoder = True) composed from the pieces of oracle/wan_ref.py the way tests/wan_full_ref.py composes `Wan` - TEST
INFRASTRUCTURE ONLY.  PARITY UNPINNED: nothing here is recorded from the reference (diffusers does not import).  Added to those
pieces: the literal mask reshuffle and the 36-channel concat of `_compute_i2v_inputs` (WanI2V/network.py:310-327); diffusers'
`WanImageEmbedding` (FP32LayerNorm - Linear - GELU (erf) - Linear - FP32LayerNorm, eps 1e-5; no pos_embed); the image branch of the
cross-attention (`add_k_proj`, `add_v_proj`, `norm_added_k`, a second softmax, the two outputs summed: Wan/network_causal.py:294-358).
The thirteen image keys and their order are read from the key map at Wan/network.py:1029-1049 and diffusers' module order (unpinned).
Runs in the dtype it is given: fp32 or fp64.  The condition is a dict {text, ff, image (optional)}."""
import dataclasses
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import wan_ref as R
import wan_full_ref as W

IMG_EMB = "transformer.condition_embedder.image_embedder."
IMG_EMB_KEYS = ("norm1.weight", "norm1.bias", "ff.net.0.proj.weight", "ff.net.0.proj.bias", "ff.net.2.weight", "ff.net.2.bias", "norm2.weight",
                "norm2.bias")
IMG_BLK_KEYS = ("attn2.add_k_proj.weight", "attn2.add_k_proj.bias", "attn2.add_v_proj.weight", "attn2.add_v_proj.bias", "attn2.norm_added_k.weight")
TINY = dataclasses.replace(R.TINY, in_channels=36)  # 2 heads, D 256, ffn 512, 2 layers, text_dim 128; 16 + 4 + 16 input channels
TINY_IMAGE_DIM = 128
LATENT = 16
MUTANTS = ("joint_softmax", "no_image", "no_norm_added_k", "mask_every_frame", "cond_before_mask", "neighbour_first_frame")


def state_dict_shapes(cfg: R.WanConfig, image_dim: int) -> Dict[str, tuple]:
    """`WanI2V.state_dict()`: `Wan`'s keys with the image embedder's eight behind text_embedder.linear_2.bias and, per block, the five
    of the image branch behind attn2.norm_k.weight.  image_dim 0: `Wan`'s keys."""
    D, out = cfg.dim, {}
    for k, shp in R.state_dict_shapes(cfg).items():
        out[k] = shp
        if not image_dim:
            continue
        if k == "transformer.condition_embedder.text_embedder.linear_2.bias":
            for n, s in zip(IMG_EMB_KEYS, ((image_dim,), (image_dim,), (image_dim, image_dim), (image_dim,), (D, image_dim), (D,), (D,), (D,))):
                out[IMG_EMB + n] = s
        if k.endswith("attn2.norm_k.weight"):
            pre = k[: -len("attn2.norm_k.weight")]
            for n, s in zip(IMG_BLK_KEYS, ((D, D), (D,), (D, D), (D,), (D,))):
                out[pre + n] = s
    return out


def random_state_dict(cfg: R.WanConfig, image_dim: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """`R.random_state_dict(cfg, seed)` (so that the keys shared with `Wan(in_channels=36)` carry the same values) plus the image keys
    from their own generator, by the same rule: fan-in scaled matrices, 0.05 biases, norm weights around 1."""
    base = R.random_state_dict(cfg, seed)
    g = torch.Generator().manual_seed(seed + 200003)
    sd = {}
    for k, shp in state_dict_shapes(cfg, image_dim).items():
        if k in base:
            sd[k] = base[k]
        elif k.endswith(("norm1.weight", "norm2.weight", "norm_added_k.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith(".bias"):
            sd[k] = 0.05 * torch.randn(shp, generator=g)
        elif k.endswith("add_k_proj.weight"):
            # keys three times the unit scale before norm_added_k: a path that skips that norm then sees logits three times as large
            # (at unit scale the RMSNorm is nearly the identity and its absence would not show)
            sd[k] = 3.0 * torch.randn(shp, generator=g) * shp[1] ** -0.5
        else:
            sd[k] = torch.randn(shp, generator=g) * shp[1] ** -0.5
    return sd


def mask_literal(B: int, Fr: int, H: int, W: int, dtype=torch.float32) -> torch.Tensor:
    """The reshuffle of WanI2V/network.py:311-325, line by line: [B, 4, F, H, W]."""
    st = 4
    num_frames = (Fr - 1) * st + 1
    m = torch.ones(B, 1, num_frames, H, W, dtype=dtype)
    m[:, :, list(range(1, num_frames))] = 0
    first = torch.repeat_interleave(m[:, :, 0:1], dim=2, repeats=st)
    m = torch.concat([first, m[:, :, 1:, :]], dim=2)
    return m.view(B, -1, st, H, W).transpose(1, 2)


def mask_first_frame(B: int, Fr: int, H: int, W: int, dtype=torch.float32) -> torch.Tensor:
    """What it reduces to: ones on latent frame 0, zeros elsewhere, on all four channels."""
    m = torch.zeros(B, 4, Fr, H, W, dtype=dtype)
    m[:, :, 0] = 1
    return m


def i2v_input(x_t: torch.Tensor, ff: torch.Tensor, mutant: Optional[str] = None) -> torch.Tensor:
    B, _, Fr, H, W = x_t.shape
    m = mask_literal(B, Fr, H, W, x_t.dtype)
    if mutant == "mask_every_frame":
        m = torch.ones_like(m)
    if mutant == "neighbour_first_frame":
        ff = torch.roll(ff, -1, dims=0)  # sample b gets b + 1's
    if mutant == "cond_before_mask":
        return torch.cat([x_t, ff, m], dim=1)
    return torch.cat([x_t, m, ff], dim=1)


def image_embedding(p, img: torch.Tensor, gelu: str = "none") -> torch.Tensor:
    """condition_embedder.image_embedder: [B, Li, image_dim] -> [B, Li, D].  gelu: "none" = exact (erf); "tanh": the mutant."""
    ie = "condition_embedder.image_embedder."
    h = R.layer_norm(img, 1e-5, p[ie + "norm1.weight"], p[ie + "norm1.bias"])
    h = F.gelu(R._lin(p, h, ie + "ff.net.0.proj"), approximate=gelu)
    return R.layer_norm(R._lin(p, h, ie + "ff.net.2"), 1e-5, p[ie + "norm2.weight"], p[ie + "norm2.bias"])


def img_kv(p, cfg: R.WanConfig, i: int, tok: torch.Tensor, norm: bool = True):
    """k_img = norm_added_k(add_k_proj(tok)), v_img = add_v_proj(tok): [B, Li, H, hd] each."""
    b = f"blocks.{i}."
    B = tok.shape[0]
    k = R._lin(p, tok, b + "attn2.add_k_proj")
    if norm:
        k = R.rms_norm(k, p[b + "attn2.norm_added_k.weight"], cfg.eps)
    return k.view(B, -1, cfg.num_heads, cfg.head_dim), R._lin(p, tok, b + "attn2.add_v_proj").view(B, -1, cfg.num_heads, cfg.head_dim)


def cross_attn_i2v(p, cfg: R.WanConfig, i: int, hs: torch.Tensor, k2, v2, ki=None, vi=None, joint: bool = False):
    """`R.cross_attn` with the image branch: (summed attention output before to_out, new stream).  ki None: the text alone.  joint:
    the mutant with ONE softmax over [img; txt]."""
    b = f"blocks.{i}."
    B, L, _ = hs.shape
    y = R.layer_norm(hs, cfg.eps, p[b + "norm2.weight"], p[b + "norm2.bias"])
    q2 = R.rms_norm(R._lin(p, y, b + "attn2.to_q"), p[b + "attn2.norm_q.weight"], cfg.eps).view(B, L, cfg.num_heads, -1)
    if ki is None:
        att = R.sdpa(q2, k2, v2)
    elif joint:
        att = R.sdpa(q2, torch.cat([ki, k2], dim=1), torch.cat([vi, v2], dim=1))
    else:
        att = R.sdpa(q2, k2, v2) + R.sdpa(q2, ki, vi)
    return att, hs + R._lin(p, att, b + "attn2.to_out.0")


class WanI2VRef:
    def __init__(self, sd: Dict[str, torch.Tensor], cfg: R.WanConfig, dtype=torch.float32, mutant: Optional[str] = None):
        assert mutant in (None,) + MUTANTS
        self.cfg, self.dtype, self.mutant = cfg, dtype, mutant
        self.p = {k[len("transformer."):]: v.to(dtype) for k, v in sd.items()}
        self.has_image = "condition_embedder.image_embedder.norm1.weight" in self.p

    def forward(self, x_t: torch.Tensor, t: torch.Tensor, cond: dict, r=None, skip_layers=None) -> torch.Tensor:
        """The raw network output.  x_t [B, 16, F, H, W]; cond: {"text", "ff", "image" (optional)}."""
        assert r is None
        cfg, p, dt, mu = self.cfg, self.p, self.dtype, self.mutant
        B, _, Fr, H, W = x_t.shape
        gh, gw = H // 2, W // 2
        ts32 = (1000.0 * t.float()).view(B, 1).expand(B, Fr).reshape(-1)
        cos, sin = R.rope_for_chunk(cfg, Fr, gh, gw, 0, dt)
        hs = R.patch_embed(p, i2v_input(x_t.to(dt), cond["ff"].to(dt), mu))
        temb = R.time_embedding(p, cfg, ts32.to(dt))
        tproj = R.time_projection(p, temb)
        ctx = R.text_embedding(p, cond["text"].to(dt))
        img = cond.get("image")
        tok = image_embedding(p, img.to(dt)) if (img is not None and self.has_image and mu != "no_image") else None
        for i in range(cfg.num_layers):
            if skip_layers is not None and i in skip_layers:
                continue
            mod = R.modulation(p, i, tproj, B, Fr)
            q, k, v = R.self_attn_qkv(p, cfg, i, hs, mod, cos, sin)
            hs = R.self_attn_out(p, i, hs, R.sdpa(q, k, v), mod)
            k2, v2 = R.cross_kv(p, cfg, i, ctx)
            ki, vi = img_kv(p, cfg, i, tok, norm=mu != "no_norm_added_k") if tok is not None else (None, None)
            hs = cross_attn_i2v(p, cfg, i, hs, k2, v2, ki, vi, joint=mu == "joint_softmax")[1]
            hs = R.ffn(p, cfg, i, hs, mod)
        return R.final_layer(p, cfg, hs, temb, Fr, gh, gw)


# the loops of tests/wan_full_ref.py pass their `text` argument through to forward(): here it is the condition dict
x0_loop = W.x0_loop
guided_sample = W.guided_sample

# ---- the case tests/test_gpu_wan_i2v.py runs; tests/test_wan_i2v_ref.py holds its mutants apart on the CPU ------------------------------
SHAPE = (2, 16, 5, 16, 24)  # 480 tokens per sample
TEXT_LEN, IMAGE_LEN = 37, 257
SEED = 71
T = (0.8, 0.45)


def case(seed: int = SEED, image_dim: int = TINY_IMAGE_DIM):
    """(state dict, x, t, cond) of the forward test.  The first-frame latents are zero past frame 0, as the reference pads them; the
    image tokens are at the scale of CLIP's penultimate layer after the embedder's own LayerNorm (unit normals)."""
    sd = random_state_dict(TINY, image_dim, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(SHAPE, generator=g)
    ff = torch.randn(SHAPE, generator=g)
    ff[:, :, 1:] = 0.25 * ff[:, :, 1:]  # (the encoded zero pixels are a non-zero latent)
    cond = {"text": torch.randn(SHAPE[0], TEXT_LEN, 128, generator=g), "ff": ff,
            "image": torch.randn(SHAPE[0], IMAGE_LEN, max(image_dim, 64), generator=g)}
    if not image_dim:
        del cond["image"]
    return sd, x, torch.tensor(T, dtype=torch.float64), cond
