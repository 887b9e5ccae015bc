"""The video-to-video network (reference fastgen/networks/VaceWan/network.py `VACEWan`, vace_classify_forward_*; block body: diffusers'
WanVACETransformerBlock as the reference calls it) composed from the pieces of oracle/wan_ref.py the way tests/wan_full_ref.py
composes `Wan` - TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED: nothing here is recorded from the reference (diffusers does not import);
the VACE keys and their order are read from diffusers' module order.  Added to those pieces: `vace_patch_embedding` and the zero
padding of its tokens (VaceWan/network.py:75-91), the VACE chain (:214-227; block 0 starts with proj_in(c) + x0, every block ends with
hint = proj_out(c), the next block continues from c) and the main loop's consumption of (hint, scale) from the front of the list
(:229-249; a skipped layer is passed over before the pop).  Runs in the dtype it is given: fp32 or fp64.  The condition is a dict
{"text", "ctx"}."""
import dataclasses
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import wan_ref as R
import wan_full_ref as W

TINY = dataclasses.replace(R.TINY, num_layers=3)  # 2 heads, D 256, ffn 512, text_dim 128; three main blocks
VACE_LAYERS = (0, 2)
VACE_IN = 96
MUTANTS = ("no_hints", "hint_by_layer_index", "no_proj_in_residual", "pad_after_proj_in", "chain_from_hint", "scale_ignored", "hint_before_block",
           "main_block_modulation")
_VB = 1000  # VACE block k's parameters are also filed as main block _VB + k, so that the block pieces of oracle/wan_ref.py serve them


def state_dict_shapes(cfg: R.WanConfig, vace_layers: Sequence[int] = VACE_LAYERS, vace_in: int = VACE_IN, r_timestep: bool = False) -> Dict[str, tuple]:
    """`VACEWan.state_dict()`: `Wan`'s keys with vace_patch_embedding.* behind patch_embedding.* and vace_blocks.{k}.* behind the last
    blocks.* key; per VACE block scale_shift_table, proj_in.* (k = 0 only), the main block's keys in their order, proj_out.*."""
    D, out = cfg.dim, {}
    base = W.state_dict_shapes(cfg, r_timestep)
    last = f"transformer.blocks.{cfg.num_layers - 1}.ffn.net.2.bias"
    for k, shp in base.items():
        out[k] = shp
        if k == "transformer.patch_embedding.bias":
            out["transformer.vace_patch_embedding.weight"] = (D, vace_in, 1, 2, 2)
            out["transformer.vace_patch_embedding.bias"] = (D,)
        if k == last:
            for j in range(len(vace_layers)):
                pre = f"transformer.vace_blocks.{j}."
                for n, s in base.items():
                    if not n.startswith("transformer.blocks.0."):
                        continue
                    leaf = n[len("transformer.blocks.0."):]
                    out[pre + leaf] = s
                    if leaf == "scale_shift_table" and j == 0:
                        out[pre + "proj_in.weight"] = (D, D)
                        out[pre + "proj_in.bias"] = (D,)
                out[pre + "proj_out.weight"] = (D, D)
                out[pre + "proj_out.bias"] = (D,)
    return out


def random_state_dict(cfg: R.WanConfig, seed: int = 0, vace_layers: Sequence[int] = VACE_LAYERS, vace_in: int = VACE_IN,
                      r_timestep: bool = False) -> Dict[str, torch.Tensor]:
    """`W.random_state_dict(cfg, seed)` (so that the keys shared with `Wan` carry the same values) plus the VACE keys from their own
    generator by the same rule - fan-in scaled matrices (proj_out among them: a hint is then as large as the stream it joins), 0.05
    biases, norm weights around 1 - with two exceptions.  A VACE block's scale_shift_table is drawn at 0.5, not at 1 / sqrt(D).  At the
    main blocks' scale the table is a small correction to timestep_proj and a VACE block that read the MAIN block's table could not be
    told from the network.  Likewise proj_in.bias is drawn at 0.5, not at 0.05: it is all that a padded row of the control stream
    carries besides x0, and at 0.05 padding behind proj_in (zero rows) could not be told from padding in front of it (bias rows)."""
    base = W.random_state_dict(cfg, seed, r_timestep=r_timestep)
    g = torch.Generator().manual_seed(seed + 300007)
    sd = {}
    for k, shp in state_dict_shapes(cfg, vace_layers, vace_in, r_timestep).items():
        if k in base:
            sd[k] = base[k]
        elif k.endswith(("norm_q.weight", "norm_k.weight", "norm2.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("scale_shift_table"):
            sd[k] = 0.5 * torch.randn(shp, generator=g)
        elif k.endswith("proj_in.bias"):
            sd[k] = 0.5 * torch.randn(shp, generator=g)
        elif k.endswith(".bias"):
            sd[k] = 0.05 * torch.randn(shp, generator=g)
        else:
            fan_in = int(torch.tensor(shp[1:]).prod())
            sd[k] = torch.randn(shp, generator=g) * fan_in ** -0.5
    return sd


def consumption_literal(num_layers: int, vace_layers: Sequence[int], skip_layers=None):
    """The pop loop of VaceWan/network.py:226-245 transcribed literally, on indices: [(main block, hint index)] in execution order."""
    lst = [(k, k) for k in range(len(vace_layers))]  # (conditioning_states of VACE block k, scale k)
    lst = lst[::-1]
    got = []
    for block_idx in range(num_layers):
        if skip_layers is not None and block_idx in skip_layers:
            continue
        if block_idx in vace_layers:
            assert lst, "Control states depleted before applying to configured layers"
            hint, scale = lst.pop()
            assert hint == scale
            got.append((block_idx, hint))
    return got


def vace_patch_embed(p, ctx: torch.Tensor) -> torch.Tensor:
    return F.conv3d(ctx, p["vace_patch_embedding.weight"], p["vace_patch_embedding.bias"], stride=(1, 2, 2)).flatten(2).transpose(1, 2)


def pad_tokens(c: torch.Tensor, L: int) -> torch.Tensor:
    return torch.cat([c, c.new_zeros(c.shape[0], L - c.shape[1], c.shape[2])], dim=1)


class WanVaceRef:
    def __init__(self, sd: Dict[str, torch.Tensor], cfg: R.WanConfig, dtype=torch.float32, vace_layers: Sequence[int] = VACE_LAYERS,
                 context_scale=1.0, time_cond_type: str = "abs", mutant: Optional[str] = None):
        assert mutant in (None,) + MUTANTS and time_cond_type in ("diff", "abs")
        self.cfg, self.dtype, self.mutant, self.vace_layers, self.time_cond_type = cfg, dtype, mutant, tuple(vace_layers), time_cond_type
        n = len(self.vace_layers)
        self.scales = [float(context_scale)] * n if isinstance(context_scale, (int, float)) else [float(s) for s in context_scale]
        assert len(self.scales) == n
        self.p = {k[len("transformer."):]: v.to(dtype) for k, v in sd.items()}
        for k, v in list(self.p.items()):
            if k.startswith("vace_blocks."):
                j, leaf = k[len("vace_blocks."):].split(".", 1)
                self.p[f"blocks.{_VB + int(j)}.{leaf}"] = v
        self.has_r = "r_embedder.time_proj.weight" in self.p

    def block(self, i: int, hs, tproj, ctx, cos, sin, B: int, Fr: int, mod_from: Optional[int] = None, taps: Optional[dict] = None):
        cfg, p = self.cfg, self.p
        mod = R.modulation(p, i if mod_from is None else mod_from, tproj, B, Fr)
        q, k, v = R.self_attn_qkv(p, cfg, i, hs, mod, cos, sin)
        att1 = R.sdpa(q, k, v)
        hs = R.self_attn_out(p, i, hs, att1, mod)
        x1 = hs
        k2, v2 = R.cross_kv(p, cfg, i, ctx)
        att2, hs = R.cross_attn(p, cfg, i, hs, k2, v2)
        x2 = hs
        hs = R.ffn(p, cfg, i, hs, mod)
        if taps is not None:
            taps.update(attn1=att1.flatten(2), x_attn1=x1, attn2=att2.flatten(2) if att2.ndim == 4 else att2, x_attn2=x2, x_ffn=hs)
        return hs

    def embed(self, x_t, t, cond, r=None):
        """(x0 tokens, temb, tproj, text context, padded control tokens before proj_in, rope)"""
        cfg, p, dt = self.cfg, self.p, self.dtype
        B, _, Fr, H, W = x_t.shape
        ts32 = (1000.0 * t.float()).view(B, 1).expand(B, Fr).reshape(-1)
        hs = R.patch_embed(p, x_t.to(dt))
        temb = R.time_embedding(p, cfg, ts32.to(dt))
        tproj = R.time_projection(p, temb)
        if r is not None:
            if not self.has_r:
                raise ValueError("r_timestep provided but no r_embedder is present")
            rs32 = (1000.0 * r.float()).view(B, 1).expand(B, Fr).reshape(-1)
            if self.time_cond_type == "diff":
                rs32 = ts32 - rs32
            pr = {k.replace("r_embedder.", "condition_embedder."): v for k, v in p.items() if k.startswith("r_embedder.")}
            remb = R.time_embedding(pr, cfg, rs32.to(dt))
            tproj = tproj + R.time_projection(pr, remb)
            temb = temb + remb
        return hs, temb, tproj, R.text_embedding(p, cond["text"].to(dt))

    def ctx_in(self, ctx: torch.Tensor, L: int) -> torch.Tensor:
        """proj_in(pad(vace_patch_embedding(ctx))): what the engine keeps per context.  A padded row is proj_in.bias."""
        p = self.p
        c = vace_patch_embed(p, ctx.to(self.dtype))
        if self.mutant == "pad_after_proj_in":
            return pad_tokens(R._lin(p, c, "vace_blocks.0.proj_in"), L)
        return R._lin(p, pad_tokens(c, L), "vace_blocks.0.proj_in")

    def forward(self, x_t: torch.Tensor, t: torch.Tensor, cond: dict, r=None, skip_layers=None) -> torch.Tensor:
        """The raw network output.  x_t [B, 16, F, H, W]; cond: {"text", "ctx" [B, 96, Fc <= F, H, W]}."""
        cfg, p, dt, mu = self.cfg, self.p, self.dtype, self.mutant
        B, _, Fr, H, W = x_t.shape
        gh, gw = H // 2, W // 2
        cos, sin = R.rope_for_chunk(cfg, Fr, gh, gw, 0, dt)
        hs, temb, tproj, text = self.embed(x_t, t, cond, r)
        hints = []
        c = self.ctx_in(cond["ctx"], hs.shape[1])
        if mu != "no_proj_in_residual":
            c = c + hs
        for j in range(len(self.vace_layers)):
            c = self.block(_VB + j, c, tproj, text, cos, sin, B, Fr, mod_from=self.vace_layers[j] if mu == "main_block_modulation" else None)
            hint = R._lin(p, c, f"vace_blocks.{j}.proj_out")
            hints.append(hint)
            if mu == "chain_from_hint":
                c = hint
        order = list(range(len(hints)))
        for i in range(cfg.num_layers):
            if skip_layers is not None and i in skip_layers:
                continue
            take = i in self.vace_layers and mu != "no_hints"
            if take:
                j = self.vace_layers.index(i) if mu == "hint_by_layer_index" else order.pop(0)
                add = hints[j] * (1.0 if mu == "scale_ignored" else self.scales[j])
                if mu == "hint_before_block":
                    hs = hs + add
            hs = self.block(i, hs, tproj, text, cos, sin, B, Fr)
            if take and mu != "hint_before_block":
                hs = hs + add
        return R.final_layer(p, cfg, hs, temb, Fr, gh, gw)


# the loops of tests/wan_full_ref.py pass their `text` argument through to forward(): here it is the condition dict
x0_loop = W.x0_loop
meanflow_loop = W.meanflow_loop
guided_sample = W.guided_sample

# ---- the cases tests/test_gpu_wan_vace.py runs; tests/test_wan_vace_ref.py holds their mutants apart on the CPU --------------------------
SHAPE = (2, 16, 5, 16, 24)  # 480 tokens per sample
TEXT_LEN = 37
SEED = 83
T = (0.8, 0.45)
SCALES = [0.5, 1.5]
# which case exposes which mutant: (context frames, skip_layers)
CASES = {"full": (5, None), "short": (3, None), "skip": (5, [0])}
EXPOSED_BY = {"no_hints": "full", "hint_by_layer_index": "skip", "no_proj_in_residual": "full", "pad_after_proj_in": "short", "chain_from_hint": "full",
              "scale_ignored": "full", "hint_before_block": "full", "main_block_modulation": "full"}


def case(name: str = "full", seed: int = SEED, r_timestep: bool = False):
    """(state dict, x, t, cond, skip_layers) of a forward case.  The context is at the scale of VAE latents next to 64 channels of ones."""
    fc, skip = CASES[name]
    sd = random_state_dict(TINY, seed, r_timestep=r_timestep)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(SHAPE, generator=g)
    text = torch.randn(SHAPE[0], TEXT_LEN, 128, generator=g)
    lat = torch.randn(SHAPE[0], 32, SHAPE[2], SHAPE[3], SHAPE[4], generator=g)
    ctx = torch.cat([lat, torch.ones(SHAPE[0], 64, SHAPE[2], SHAPE[3], SHAPE[4])], dim=1)[:, :, :fc].contiguous()
    return sd, x, torch.tensor(T, dtype=torch.float64), {"text": text, "ctx": ctx}, skip
