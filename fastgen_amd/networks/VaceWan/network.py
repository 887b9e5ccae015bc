"""`VACEWan` drop-in for the reference's `fastgen.networks.VaceWan.network.VACEWan` (`VACE_Wan_1_3B_Config` / `VACE_Wan_14B_Config`): the
video-to-video network - the bidirectional video DiT (`fastgen_amd.networks.Wan.network.Wan`) with a second stack of "VACE blocks"
that reads a 96-channel control video (`condition["vid_context"]`: inactive | reactive latents | 64 mask channels) and adds scaled hints
into the main token stream behind the layers in `vace_layers` - backed by `fg_wan_create_vace`, `fg_wan_set_vace_context`,
`fg_wan_set_vace_scale` and `Wan`'s entry points on that handle.

The condition is a dict: `text_embeds` [B, L, text_dim] and `vid_context` [B, vace_in_channels, Fc, H, W] with Fc <= F (the embedded
context is zero-padded to the video's token count) and the video's H, W.  It is handed to the engine once per (tensor object, version,
shape), like the text; new contents at the same shape replay the fused loops' graphs.  `context_scale` (a float, or one value per VACE
layer) is read at every call, as the reference reads it; under `skip_layers` the j-th EXECUTED VACE layer receives hint j with scale j -
the reference pops (hint, scale) from the front of its list behind the skip test, and this reproduces that order.

PARITY UNPINNED like `Wan`; in addition the VACE keys (`transformer.vace_patch_embedding.*` behind `transformer.patch_embedding.*`,
`transformer.vace_blocks.{k}.*` behind the last `transformer.blocks.*` key; per block scale_shift_table, proj_in.* for k = 0 only, the
main block's keys, proj_out.*) follow diffusers' module order as read, the block body is diffusers' WanVACETransformerBlock as read,
and the published `vace_layers` (1.3B: 30 layers, 0, 2, ..., 28; 14B: 40 layers, 0, 5, ..., 35) are quoted, not checked - they are
constructor keywords (`vace_layers=None`: every second layer, the 1.3B pattern).

Raises (never falls back): everything `Wan` raises, `CausalVACEWan`, a context whose H / W differ from the video's or with more frames
than the video, `prepare_vid_conditioning` without ready-made latents (the depth annotator and the VAE are outside this project)."""
from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Sequence, Union

import torch

from fastgen_amd import _lib
from fastgen_amd.networks._engine import ptr
from fastgen_amd.networks.Wan._shared import ConditionSlot
from fastgen_amd.networks.Wan.network import Wan


class VACEWan(Wan):
    is_vid2vid = True
    _SLOTS = ("text", "vace")  # (packing invalidates the context - proj_in, vace_patch_embedding - together with the text)

    def __init__(self, num_attention_heads: int = 12, attention_head_dim: int = 128, in_channels: int = 16, out_channels: int = 16,
                 text_dim: int = 4096, freq_dim: int = 256, ffn_dim: int = 8960, num_layers: int = 30,
                 vace_layers: Optional[Sequence[int]] = None, vace_in_channels: int = 96, context_scale: Union[float, List[float]] = 1.0,
                 depth_model_path: Optional[str] = None, time_cond_type: str = "abs", **kwargs):
        layers = list(range(0, num_layers, 2)) if vace_layers is None else [int(i) for i in vace_layers]
        if not 1 <= len(layers) <= 64 or any(b <= a for a, b in zip(layers, layers[1:])) or layers[0] < 0 or layers[-1] >= num_layers:
            raise ValueError(f"vace_layers must be 1 .. 64 strictly ascending block indices in [0, {num_layers}), got {layers}")
        if not 0 < int(vace_in_channels) <= 128:
            raise ValueError(f"vace_in_channels must be in (0, 128], got {vace_in_channels}")
        v = _lib.fg_wan_vace_config()
        v.vace_in_channels, v.num_vace_layers = int(vace_in_channels), len(layers)
        for j, i in enumerate(layers):
            v.vace_layers[j] = i
        self._vace_cfg, self._scale_slot = v, ConditionSlot()  # (the scales outlive a packing)
        self.vace_layers, self.vace_in_channels = tuple(layers), int(vace_in_channels)
        self.context_scale, self.depth_model_path = context_scale, depth_model_path
        self._all_zero_latent = None
        super().__init__(num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim, in_channels=in_channels,
                         out_channels=out_channels, text_dim=text_dim, freq_dim=freq_dim, ffn_dim=ffn_dim, num_layers=num_layers,
                         time_cond_type=time_cond_type, **kwargs)

    def _build_engine(self, **kw) -> None:
        super()._build_engine(vace=self._vace_cfg, **kw)

    # ---- the reference's helpers -------------------------------------------------------------------------------------------
    @staticmethod
    def vace_context(inactive_latents: torch.Tensor, reactive_latents: torch.Tensor) -> torch.Tensor:
        """The control video of `prepare_vid_conditioning` (VaceWan/network.py:570-579) from ready-made latents: [inactive | reactive |
        64 channels of ones] - [B, 96, F, H, W] for two 16-channel latents."""
        video_latents = torch.cat([inactive_latents, reactive_latents.to(inactive_latents.device, inactive_latents.dtype)], dim=1)
        b, _, t, h, w = video_latents.shape
        return torch.cat([video_latents, torch.ones(b, 64, t, h, w, device=video_latents.device, dtype=video_latents.dtype)], dim=1)

    def prepare_vid_conditioning(self, video: torch.Tensor, condition_latents: Optional[torch.Tensor] = None) -> torch.Tensor:
        """With `condition_latents` (the reactive latents) and the encoded all-zero video in `self._all_zero_latent` (the reference
        encodes it with its VAE on first use): `vace_context` of the two.  Anything that needs the depth annotator or the VAE raises."""
        if condition_latents is None:
            raise NotImplementedError("prepare_vid_conditioning without condition_latents needs the depth annotator and the VAE, which are "
                                      "outside this project: build the context with VACEWan.vace_context(inactive_latents, reactive_latents)")
        if self._all_zero_latent is None:
            raise NotImplementedError("the inactive latents are the VAE encoding of an all-zero video (VaceWan/network.py:561-565) and the VAE is "
                                      "outside this project: set `_all_zero_latent`, or call VACEWan.vace_context(inactive_latents, reactive_latents)")
        return self.vace_context(self._all_zero_latent.to(video.device, video.dtype), condition_latents.to(video.device, video.dtype))

    # ---- the condition -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _split_condition(condition: Any, what: str = "condition"):
        assert isinstance(condition, dict), f"{what} must be a dict"  # (the reference's asserts, VaceWan/network.py:679-681)
        assert "text_embeds" in condition, f"{what} must contain 'text_embeds'"
        assert "vid_context" in condition, f"{what} must contain 'vid_context'"
        text = condition["text_embeds"]
        return (torch.stack(text, dim=0) if isinstance(text, list) else text), (condition["vid_context"],)

    def _scales(self) -> List[float]:
        """`control_hidden_states_scale` as `VACEWan.forward` forms it (VaceWan/network.py:698-715), with its error texts."""
        s, n = self.context_scale, len(self.vace_layers)
        if isinstance(s, (int, float)):
            s = [s] * n
        if isinstance(s, list):
            if len(s) != n:
                raise ValueError(f"Length of `control_hidden_states_scale` {len(s)} does not match number of layers {n}.")
            s = torch.tensor(s)
        if isinstance(s, torch.Tensor):
            if s.size(0) != n:
                raise ValueError(f"Length of `control_hidden_states_scale` {s.size(0)} does not match number of layers {n}.")
            return [float(v) for v in s.detach().cpu().reshape(-1).tolist()]
        raise TypeError(f"context_scale must be a number, a list or a tensor, got {type(s).__name__}")

    def _set_scales(self, dev) -> None:
        s = self._scales()
        if self._scale_slot.same(extra=s):
            return
        _lib.check(_lib.lib().fg_wan_set_vace_scale(self._h, (ctypes.c_float * len(s))(*s), len(s), self._stream(dev)))
        self._scale_slot.remember(extra=s)

    def _set_context(self, ctx: torch.Tensor, B: int, F: int, H: int, W: int, dev) -> None:
        """The control video into the handle, once per (tensor object, version, shape) as `_set_text`."""
        C = self.vace_in_channels
        if ctx.ndim != 5 or tuple(ctx.shape[:2]) != (B, C):
            raise ValueError(f"vid_context must be [{B}, {C}, Fc, H, W], got {tuple(ctx.shape)}")
        if tuple(ctx.shape[3:]) != (H, W):
            raise ValueError(f"vid_context is {ctx.shape[3]}x{ctx.shape[4]}, the video {H}x{W}: the context must have the video's height and width")
        if not 1 <= ctx.shape[2] <= F:
            raise ValueError(f"vid_context has {ctx.shape[2]} frames, the video {F}: a context with more frames than the video is not implemented")
        slot = self._slots["vace"]
        if slot.same(ctx, extra=(F,)):
            return
        c32 = ctx.detach().to(device=dev, dtype=torch.float32).contiguous()
        L = _lib.lib()
        ws = self._eng.workspace(("vace", self._cfg.compute_dtype), L.fg_wan_vace_context_workspace_bytes(self._h, B, F, H, W), dev)
        _lib.check(L.fg_wan_set_vace_context(self._h, ptr(c32), B, F, ctx.shape[2], H, W, ptr(ws), ws.numel(), self._stream(dev)))
        slot.remember(ctx, extra=(F,))

    def _set_rest(self, rest, B: int, F: int, H: int, W: int, dev) -> None:
        self._set_scales(dev)  # (read at every call, as the reference reads `context_scale`)
        self._set_context(*rest, B, F, H, W, dev)

    def _sample_rest(self, rest, neg_rest, dev):
        if neg_rest is None:
            return rest
        (ctx,), (nctx,) = rest, neg_rest
        if nctx.shape != ctx.shape:
            raise ValueError(f"neg_condition's vid_context {tuple(nctx.shape)} must be shaped like condition's {tuple(ctx.shape)}")
        return (torch.cat([ctx.to(dev), nctx.to(dev)], dim=0),)

    # ---- calls: `Wan`'s, under the control video (a new context or new scales at the same shapes replay the fused loops' graphs) ----
    def forward(self, x_t: torch.Tensor, t: torch.Tensor, condition: Optional[Dict[str, torch.Tensor]] = None, r: Optional[torch.Tensor] = None,
                **kwargs):
        self._scales()  # (the reference's length check comes before the transformer runs)
        return super().forward(x_t, t, condition=condition, r=r, **kwargs)

    @torch.no_grad()
    def sample(self, noise: torch.Tensor, condition: Optional[Dict[str, torch.Tensor]] = None,
               neg_condition: Optional[Dict[str, torch.Tensor]] = None, guidance_scale: Optional[float] = 5.0, num_steps: int = 50,
               shift: float = 16.0, **kwargs) -> torch.Tensor:
        """`VACEWan.sample` (VaceWan/network.py:626-641: `Wan.sample` with guidance_scale 5.0, 50 steps, shift 16.0) over `Wan.sample`'s
        one call: when guided, the stacked batch [x; x] runs against the text and the control video of [condition; neg_condition]."""
        return super().sample(noise, condition=condition, neg_condition=neg_condition, guidance_scale=guidance_scale, num_steps=num_steps,
                              shift=shift, **kwargs)


class CausalVACEWan:
    """The reference's causal VACE network is not implemented: the chunked and causal entry points refuse a VACE handle."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("CausalVACEWan is not implemented: VACE runs on the bidirectional network (VACEWan) only")
