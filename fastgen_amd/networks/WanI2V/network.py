"""`WanI2V` drop-in for the reference's `fastgen.networks.WanI2V.network.WanI2V` in the Wan2.1-I2V convention (`concat_mask=True`,
`use_image_encoder=True`): the bidirectional video DiT (`fastgen_amd.networks.Wan.network.Wan`) on the 36-channel input
[x_t | 4 mask channels | first_frame_cond] with the CLIP image tokens' embedder and a second, separately normalised cross-attention
softmax over the image keys in every block - backed by `fg_wan_create_i2v`, `fg_wan_set_i2v_cond` and `Wan`'s entry points on that
handle.  The network of configs/experiments/WanI2V/config_dmd2_14b.py / config_sft_14b.py and the teacher of the I2V students.

The condition is a dict: `text_embeds` [B, L, text_dim], `first_frame_cond` [B, 16, F, H, W] and, optionally,
`encoder_hidden_states_image` [B, 257, image_dim] (absent, or `image_dim=0`: no image context - the blocks run the text attention alone).
It is handed to the engine once per (tensor objects, versions, shapes), like the text; new first-frame contents or image tokens at
the same shapes replay the fused loops' graphs (the handle's buffers are rewritten in place).

PARITY UNPINNED like `Wan`; in addition the thirteen image keys (`transformer.condition_embedder.image_embedder.*`, per block
`attn2.add_k_proj.*`, `attn2.add_v_proj.*`, `attn2.norm_added_k.weight`) and their order are read from the reference's key map
(Wan/network.py:1029-1049) and diffusers' module order, not recorded from a run.

The Wan2.2-TI2V convention (`concat_mask=False, use_image_encoder=False, expand_timesteps=True`: Wan2.2-TI2V-5B, the network of
configs/experiments/WanI2V/config_{dmd2,sft}_wan22_5b.py) runs on `fg_wan_create_ti2v` / `fg_wan_set_first_frame`: `Wan`'s state dict (no
image keys), `in_channels == out_channels` (48), the condition `{"text_embeds", "first_frame_cond"}` with `first_frame_cond`
[B, C, 1, H, W] (or [B, C, F, H, W], of which only frame 0 is read).  Frame 0 of the network's input is the condition's, frame 0's
timestep (and r) is zero, frame 0 of every result - `forward` whatever `fwd_pred_type`, `few_step_sample`, `sample` - is the condition's,
and `preserve_conditioning` does the replacement.  PARITY UNPINNED like everything here.

Raises (never falls back): everything `Wan` raises, any other mixture of the three flags, the MeanFlow loop on the TI2V convention, the
image embedder's `pos_embed` (FLF2V)."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch

from fastgen_amd import _lib
from fastgen_amd.networks._engine import ptr
from fastgen_amd.networks.Wan.network import Wan

_MASK_CHANNELS = 4  # scale_factor_temporal of the Wan VAE (WanI2V/network.py:312)


class WanI2V(Wan):
    is_i2v = True
    # the reference's hook returns x unchanged under concat_mask (the first frame is part of the network's input, not of the latents):
    # FastGenModel.generator_fn may keep the fused loop
    preserve_conditioning_is_identity = True
    # (an instance attribute, False, on the Wan2.2 TI2V convention, where the hook replaces frame 0.)  There the engine replaces it too:
    # the network reads the condition in frame 0's place and every prediction carries it, which leaves the hook's effect on
    # intermediate states unobservable in the result (tests/test_gpu_wan_ti2v.py: bit-equal to the generic loop), so
    # FastGenModel.generator_fn keeps the fused loop for a network that sets this
    fused_loop_preserves_conditioning = True
    _SLOTS = ("text", "i2v")  # (packing invalidates the image-to-video condition together with the text)

    def __init__(self, num_attention_heads: int = 40, attention_head_dim: int = 128, in_channels: int = 36, out_channels: int = 16,
                 text_dim: int = 4096, freq_dim: int = 256, ffn_dim: int = 13824, num_layers: int = 40, image_dim: Optional[int] = 1280,
                 concat_mask: bool = True, use_image_encoder: bool = True, expand_timesteps: bool = False, pos_embed_seq_len: Optional[int] = None,
                 **kwargs):
        flags = (bool(concat_mask), bool(use_image_encoder), bool(expand_timesteps))
        self.is_ti2v = flags == (False, False, True)
        if not self.is_ti2v and (not concat_mask or expand_timesteps):
            raise NotImplementedError(f"concat_mask={concat_mask}, use_image_encoder={use_image_encoder}, expand_timesteps={expand_timesteps} is "
                                      "not implemented: WanI2V serves Wan2.1 I2V (concat_mask=True, expand_timesteps=False) and Wan2.2 TI2V "
                                      "(concat_mask=False, use_image_encoder=False, expand_timesteps=True)")
        if pos_embed_seq_len is not None:
            raise NotImplementedError("pos_embed of the image embedder (pos_embed_seq_len, FLF2V) is not implemented")
        if self.is_ti2v:
            if in_channels != out_channels:
                raise ValueError(f"Wan2.2 TI2V: in_channels {in_channels} must equal out_channels {out_channels} (no mask or condition channels)")
            if image_dim:
                raise ValueError(f"Wan2.2 TI2V has no image encoder: image_dim must be None, got {image_dim}")
            ti2v = _lib.fg_wan_ti2v_config()
            ti2v.latent_channels = out_channels
            self._i2v_cfg, self._ti2v_cfg = None, ti2v
            self.concat_mask, self.use_image_encoder, self.image_dim, self.latent_channels = False, False, 0, out_channels
            self.preserve_conditioning_is_identity, self.fused_loop_preserves_conditioning = False, True
            super().__init__(num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim, in_channels=in_channels,
                             out_channels=out_channels, text_dim=text_dim, freq_dim=freq_dim, ffn_dim=ffn_dim, num_layers=num_layers,
                             expand_timesteps=True, **kwargs)
            return
        self._ti2v_cfg = None
        i2v = _lib.fg_wan_i2v_config()
        i2v.latent_channels, i2v.mask_channels, i2v.image_dim = out_channels, _MASK_CHANNELS, int(image_dim or 0)
        self._i2v_cfg = i2v
        self.concat_mask, self.use_image_encoder, self.image_dim = True, bool(use_image_encoder), int(image_dim or 0)
        self.latent_channels = out_channels
        super().__init__(num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim, in_channels=in_channels,
                         out_channels=out_channels, text_dim=text_dim, freq_dim=freq_dim, ffn_dim=ffn_dim, num_layers=num_layers, **kwargs)

    def _build_engine(self, **kw) -> None:
        super()._build_engine(i2v=self._i2v_cfg, ti2v=self._ti2v_cfg, **kw)

    # ---- the reference's surface -------------------------------------------------------------------------------------------
    def preserve_conditioning(self, x: torch.Tensor, condition: Any) -> torch.Tensor:
        """`WanI2V.preserve_conditioning` (WanI2V/network.py:228-252).  Under concat_mask the latents carry no conditioning frame and x is
        returned as it is; Wan2.2 TI2V: a clone of x with frame 0 set from the condition's `first_frame_cond`."""
        if self.concat_mask or not isinstance(condition, dict) or "first_frame_cond" not in condition:
            return x
        x = x.clone()
        x[:, :, 0] = condition["first_frame_cond"][:, :, 0].to(device=x.device, dtype=x.dtype)
        return x

    # ---- the condition -----------------------------------------------------------------------------------------------------
    @property
    def _video_channels(self) -> int:
        return self.latent_channels

    @staticmethod
    def _split_condition(condition: Any, what: str = "condition"):
        assert isinstance(condition, dict), f"{what} must be a dict"  # (the reference's asserts, WanI2V/network.py:457-459)
        assert "text_embeds" in condition, f"{what} must contain 'text_embeds'"
        assert "first_frame_cond" in condition, f"{what} must contain 'first_frame_cond'"
        text = condition["text_embeds"]
        text = torch.stack(text, dim=0) if isinstance(text, list) else text
        return text, (condition["first_frame_cond"], condition.get("encoder_hidden_states_image"))

    def _set_first_frame(self, ff: torch.Tensor, B: int, F: int, H: int, W: int, dev) -> None:
        """Wan2.2 TI2V: frame 0 of `first_frame_cond` into the handle, once per (tensor object, version, shape) as `_set_text`."""
        C = self.latent_channels
        if ff.ndim != 5 or tuple(ff.shape[:2]) != (B, C) or ff.shape[2] not in (1, F) or tuple(ff.shape[3:]) != (H, W):
            raise ValueError(f"first_frame_cond must be {(B, C, 1, H, W)} (or {(B, C, F, H, W)}: only frame 0 is read), got {tuple(ff.shape)}")
        slot = self._slots["i2v"]
        if slot.same(ff):
            return
        ff32 = ff.detach()[:, :, :1].to(device=dev, dtype=torch.float32).contiguous()
        _lib.check(_lib.lib().fg_wan_set_first_frame(self._h, ptr(ff32), B, H, W, self._stream(dev)))
        slot.remember(ff)

    def _set_i2v(self, ff: torch.Tensor, image: Optional[torch.Tensor], B: int, F: int, H: int, W: int, dev) -> None:
        """First-frame latents and image tokens into the handle, once per (tensor objects, versions, shapes) as `_set_text`."""
        if self.is_ti2v:
            return self._set_first_frame(ff, B, F, H, W, dev)
        if self.image_dim == 0 or not self.use_image_encoder:
            image = None
        if tuple(ff.shape) != (B, self.latent_channels, F, H, W):
            raise ValueError(f"first_frame_cond must be {(B, self.latent_channels, F, H, W)} (zero-padded to the video's frames), got {tuple(ff.shape)}")
        if image is not None and (image.ndim != 3 or image.shape[0] != B or image.shape[2] != self.image_dim or not 1 <= image.shape[1] <= 1024):
            raise ValueError(f"encoder_hidden_states_image must be [{B}, 1 .. 1024, {self.image_dim}], got {tuple(image.shape)}")
        slot = self._slots["i2v"]
        if slot.same(ff, image):
            return
        ff32 = ff.detach().to(device=dev, dtype=torch.float32).contiguous()
        im32 = None if image is None else image.detach().to(device=dev, dtype=torch.float32).contiguous()
        L = _lib.lib()
        Li = 0 if im32 is None else im32.shape[1]
        ws = None
        if Li:
            ws = self._eng.workspace(("i2v", self._cfg.compute_dtype), L.fg_wan_i2v_cond_workspace_bytes(self._h, B, Li), dev)
        _lib.check(L.fg_wan_set_i2v_cond(self._h, ptr(ff32), ptr(im32), B, F, H, W, Li, ptr(ws), ws.numel() if ws is not None else 0,
                                         self._stream(dev)))
        slot.remember(ff, image)

    def _set_rest(self, rest, B: int, F: int, H: int, W: int, dev) -> None:
        self._set_i2v(*rest, B, F, H, W, dev)

    def _sample_rest(self, rest, neg_rest, dev):
        ff, image = rest
        if self.is_ti2v:
            ff = ff[:, :, :1]  # (only frame 0 is read; the stacked tensor below is a fresh one either way)
        if neg_rest is not None:
            nff, nimage = neg_rest
            if (image is None) != (nimage is None):
                raise ValueError("condition and neg_condition must both carry encoder_hidden_states_image, or neither")
            ff = torch.cat([ff.to(dev), (nff[:, :, :1] if self.is_ti2v else nff).to(dev)], dim=0)
            image = None if image is None else torch.cat([image.to(dev), nimage.to(dev)], dim=0)
        return ff, image

    # ---- calls -------------------------------------------------------------------------------------------------------------
    def forward(self, x_t: torch.Tensor, t: torch.Tensor, condition: Optional[Dict[str, torch.Tensor]] = None, r: Optional[torch.Tensor] = None,
                **kwargs):
        out = super().forward(x_t, t, condition=condition, r=r, **kwargs)
        if self.is_ti2v:
            # `_replace_first_frame` behind convert_model_output (WanI2V/network.py:506-510): the conversion ran on the caller's x_t, the
            # condition's frame 0 lands last whatever fwd_pred_type is (the engine wrote it into the raw output already)
            out[:, :, 0] = condition["first_frame_cond"][:, :, 0].to(device=out.device, dtype=out.dtype)
        return out

    def supports_fused_loop(self, kind: str) -> bool:
        # (the MeanFlow loop would write the first-frame latents into a velocity: refused by the engine on this convention)
        return super().supports_fused_loop(kind) and not (self.is_ti2v and kind == "meanflow")

    @torch.no_grad()
    def sample(self, noise: torch.Tensor, condition: Optional[Dict[str, torch.Tensor]] = None,
               neg_condition: Optional[Dict[str, torch.Tensor]] = None, guidance_scale: Optional[float] = 5.0, num_steps: int = 40,
               shift: float = 3.0, skip_layers: Optional[List[int]] = None, skip_layers_start_percent: float = 0.0, **kwargs) -> torch.Tensor:
        """`WanI2V.sample` (WanI2V/network.py:344-419) over `Wan.sample`'s one call: when guided, the stacked batch [x; x] runs against
        the text, first frame and image tokens of [condition; neg_condition].  Wan2.2 TI2V: frame 0 of the latents is `condition`'s
        after every solver step (the engine restores it), so the returned latents carry it."""
        return super().sample(noise, condition=condition, neg_condition=neg_condition, guidance_scale=guidance_scale, num_steps=num_steps,
                              shift=shift, skip_layers=skip_layers, skip_layers_start_percent=skip_layers_start_percent, **kwargs)
