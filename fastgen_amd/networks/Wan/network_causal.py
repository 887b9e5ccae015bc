"""`CausalWan` drop-in for the reference's `fastgen.networks.Wan.network_causal.CausalWan` (the causal video DiT that
`CausVidModel._student_sample_loop` drives chunk by chunk, fastgen/methods/distribution_matching/causvid.py:87-185), backed by
libfastgen_amd.so (`fg_wan_*`: bf16 token GEMMs on gemm.hip, per-frame adaLN, RMSNorm + RoPE with a frame offset, KV-cache
attention, output projection - fastgen_amd/csrc/wan.hip, engine_wan.inc).

The reference builds its transformer with `WanTransformer3DModel.from_pretrained(model_id)` (Wan/network.py:641-693: hub
weights and config, unavailable offline); here the fields of that config are constructor keywords (defaults = Wan2.1-T2V-1.3B) and
the parameters carry the same state-dict keys (`transformer.` + diffusers' names), so a converted checkpoint loads with
`load_state_dict`.  PARITY UNPINNED (the arithmetic lives in un-vendored diffusers: oracle/wan_ref.py restates it).

Autoregressive inference (`is_ar=True`, cache tags "pos" and "neg": one cache set each, the second allocated on first use), the
guided teacher sampler `sample` (classifier-free guidance over the stacked batch [cond; neg_cond], one library call:
`fg_wan_guided_sampler_run`; solver coefficients from Wan/solvers.py, unpinned like the rest), the teacher- / diffusion-forcing forward over all total_num_frames frames
(`is_ar=False`: block-wise causal mask, per-frame timesteps [B, F]), and the whole chunk-by-chunk student loop as one library call
replayed as per-chunk hipGraphs (`student_sample` -> `fg_wan_sampler_run`; CausVidModel / SelfForcingModel call it).  Raises (never falls back): autograd,
feature taps, r / image conditioning, `is_ar=False` on fewer frames, any device but a HIP GPU.

`compute_dtype="fp8"` (keyword only; default None = "bf16"): the six linears of every block that read the video tokens contract e4m3fn
operands - weights quantised per output channel at every pack, activations per token - through every call above; the text side, the
embedders, attention and the caches stay bf16.  What it costs and buys: DESIGN.md, section 10.
"""
from __future__ import annotations

import ctypes
from typing import Any, Optional, Set

import torch

from fastgen_amd import _lib
from fastgen_amd.networks._engine import ptr
from fastgen_amd.networks.Wan._shared import WanEngineNetwork
from fastgen_amd.networks.network import _fused_sample_args
from fastgen_amd.networks.noise_schedule import NET_PRED_TYPES


class CausalWan(WanEngineNetwork):
    _NAME = "CausalWan"
    CACHE_TAGS = {"pos": 0, "neg": 1}
    _SLOTS = tuple(CACHE_TAGS)  # one text per cache tag

    def __init__(self, num_attention_heads: int = 12, attention_head_dim: int = 128, in_channels: int = 16, out_channels: int = 16,
                 text_dim: int = 4096, freq_dim: int = 256, ffn_dim: int = 8960, num_layers: int = 30, eps: float = 1e-6,
                 rope_max_seq_len: int = 1024, r_timestep: bool = False, net_pred_type: str = "flow", schedule_type: str = "rf",
                 chunk_size: int = 3, total_num_frames: int = 21, enable_logvar_linear: bool = True, *,
                 compute_dtype: Optional[str] = None, **model_kwargs):
        # compute_dtype: None / "bf16" - every GEMM on bf16 operands; "fp8" - the six linears of a block that read the video tokens on
        # e4m3fn operands (include/fastgen_amd.h, fg_wan_config).  Fixed at construction; the state dict (fp32 masters) is the same.
        self._check_compute_dtype(compute_dtype, ffn_dim, "causal video DiT")
        self._pop_reference_knobs(model_kwargs)
        super().__init__(net_pred_type=net_pred_type, schedule_type=schedule_type, **model_kwargs)
        if r_timestep:
            raise NotImplementedError("r_timestep=True (a second time embedder) is not implemented for the causal video DiT path")
        self.chunk_size, self.total_num_frames = chunk_size, total_num_frames
        self._build_engine(num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim, in_channels=in_channels,
                           out_channels=out_channels, text_dim=text_dim, freq_dim=freq_dim, ffn_dim=ffn_dim, num_layers=num_layers, eps=eps,
                           rope_max_seq_len=rope_max_seq_len, chunk_size=chunk_size, total_num_frames=total_num_frames,
                           compute_dtype=compute_dtype, enable_logvar_linear=enable_logvar_linear)
        self._tag = "pos"  # the selected cache tag ("pos" outside a forward(cache_tag="neg") call)

    # ---- library plumbing (the rest: WanEngineNetwork) -----------------------------------------------------------------------
    @property
    def _text_slot(self):
        return self._slots[self._tag]

    def _check_video(self, x: torch.Tensor, what: str):
        B, C, F, H, W = x.shape
        if C != self.in_channels:
            raise ValueError(f"{what} must have {self.in_channels} channels, got {C}")
        return B, F, H, W

    def clear_caches(self) -> None:
        """`CausalWan.clear_caches` (network_causal.py:1030-1054)."""
        if torch.cuda.is_available():
            _lib.check(_lib.lib().fg_wan_clear_caches(self._h, self._stream(torch.device("cuda", torch.cuda.current_device()))))
        self._forget_text()

    def _select_tag(self, tag: str) -> None:
        """Make `tag`'s cache set (and its text slot) the one the library calls and `_set_text` act on."""
        _lib.check(_lib.lib().fg_wan_select_cache_tag(self._h, self.CACHE_TAGS[tag]))
        self._tag = tag

    def forward(self, x_t: torch.Tensor, t: torch.Tensor, condition: Optional[Any] = None, r: Optional[torch.Tensor] = None,
                return_features_early: bool = False, feature_indices: Optional[Set[int]] = None, return_logvar: bool = False,
                unpatchify_features: bool = True, fwd_pred_type: Optional[str] = None, skip_layers=None, cache_tag: str = "pos",
                cur_start_frame: int = 0, store_kv: bool = False, is_ar: bool = False, **fwd_kwargs):
        if feature_indices or return_features_early or return_logvar or skip_layers or r is not None:
            raise NotImplementedError("feature taps / logvar / skip_layers / r are not implemented for the causal video DiT path")
        if fwd_kwargs:
            raise TypeError(f"unexpected forward kwargs: {sorted(fwd_kwargs)}")
        if not is_ar and x_t.shape[2] != self.total_num_frames:
            # (the reference builds its block mask only for a call over all total_num_frames frames, network_causal.py:673-680)
            raise NotImplementedError(f"is_ar=False (block-wise causal mask) takes all total_num_frames = {self.total_num_frames} frames, got "
                                      f"{x_t.shape[2]}; chunks go through the autoregressive call (is_ar=True)")
        if cache_tag not in self.CACHE_TAGS:
            raise NotImplementedError(f"cache_tag {cache_tag!r}: the cache tags 'pos' and 'neg' are implemented")
        if fwd_pred_type is None:
            fwd_pred_type = self.net_pred_type
        else:
            assert fwd_pred_type in NET_PRED_TYPES, f"{fwd_pred_type} is not supported as fwd_pred_type"
        self._no_autograd(x_t)
        condition = self._text(condition, who="CausalWan.forward")
        B, F, H, W, dev, ws = self._setup(x_t, "x_t", _lib.lib().fg_wan_workspace_bytes, bad="bad chunk shape: {}")
        self._select_tag(cache_tag)  # the tag's own caches and text around the call; "pos" is selected again whatever happens
        try:
            out = self._forward_selected(x_t, t, condition, B, F, H, W, dev, ws, is_ar, cur_start_frame, store_kv)
        finally:
            self._select_tag("pos")
        out = out.to(x_t.dtype)
        t_in = torch.atleast_1d(t.detach()).to(dev)
        t_conv = t_in[:, None, :, None, None] if t_in.ndim == 2 else t_in
        return self.noise_scheduler.convert_model_output(x_t, out, t_conv, src_pred_type=self.net_pred_type, target_pred_type=fwd_pred_type)

    def _forward_selected(self, x_t, t, condition, B, F, H, W, dev, ws, is_ar, cur_start_frame, store_kv) -> torch.Tensor:
        """The network call on the selected cache tag: the raw fp32 output."""
        L = _lib.lib()
        self._set_text(condition, B, dev, ws)
        ts = self._frame_rows(self.noise_scheduler.rescale_t(torch.atleast_1d(t.detach()).to(dev)), B, F)
        x32 = x_t.detach().to(torch.float32).contiguous()
        out = torch.empty_like(x32)
        if is_ar:
            _lib.check(L.fg_wan_forward(self._h, ptr(x32), ptr(ts), ptr(out), B, F, H, W, int(cur_start_frame), int(bool(store_kv)), ptr(ws),
                                        ws.numel(), self._stream(dev)))
        else:  # teacher / diffusion forcing: all frames under the block-wise causal mask, caches untouched
            _lib.check(L.fg_wan_forward_block_causal(self._h, ptr(x32), ptr(ts), ptr(out), B, F, H, W, ptr(ws), ws.numel(), self._stream(dev)))
        return out

    # ---- the chunk-by-chunk student loop as one library call ------------------------------------------------------------------
    @torch.no_grad()
    def student_sample(self, x: torch.Tensor, t_list, condition: Any, sample_type: str = "sde", context_noise: float = 0.0,
                       eps: Optional[torch.Tensor] = None, seed: Optional[int] = None, use_graph: bool = True, prefill_frames: int = 0,
                       exit_steps=None) -> torch.Tensor:
        """`CausVidModel._student_sample_loop` (fastgen/methods/distribution_matching/causvid.py:87-185) over `fg_wan_sampler_run`: x
        [B, C, F, H, W] latents (already scaled to t_list[0]) are overwritten chunk by chunk with the generated frames - per chunk N x {x0
        prediction over the cached frames + this chunk; re-noise to the next timestep}, then the cache-fill call.  prefill_frames: frames at
        the head that only fill the caches (`generator_fn_extrapolation`'s bridged segment head); exit_steps: one exit index per chunk
        (`SelfForcingModel.rollout_with_gradient`).  eps: noise videos to inject instead of device draws, [steps - 1 (+ 1 if context_noise
        > 0), B, C, F, H, W].  The caches are empty afterwards, as after the reference's loop."""
        # (the count includes the context-noise video; checked here only for this call's own message: the shared check then passes)
        n_eps = max(len(t_list) - 2, 0) + (1 if context_noise and context_noise > 0 else 0)
        if eps is not None and eps.numel() != n_eps * x.numel():
            raise ValueError(f"eps must hold {n_eps} noise videos shaped like x")
        x32, steps, tl_arr, eps, seed = _fused_sample_args(x, t_list, sample_type, eps, seed, n_eps)
        if self.net_pred_type not in ("flow", "x0"):
            raise NotImplementedError(f"net_pred_type {self.net_pred_type!r} has no fused loop")
        condition = self._text(condition, who="CausalWan")
        L = _lib.lib()
        B, F, H, W, dev, ws = self._setup(x, "x", L.fg_wan_sampler_workspace_bytes)
        self._set_text(condition, B, dev, ws)
        sc = self._sampler_config(context_noise, prefill_frames)
        ex = None
        if exit_steps is not None:
            ex = (ctypes.c_int * len(exit_steps))(*[int(e) for e in exit_steps])
            n_chunks = max(1, F // self.chunk_size)
            if len(exit_steps) < n_chunks:
                raise ValueError(f"exit_steps must hold one index per chunk ({n_chunks})")
        # the latents and the injected noise are in the chunk graphs' keys by address: the loop runs on the handle's staging tensors,
        # so that a second call with the same shapes replays the graphs whatever tensors the caller passes
        dt = self._cfg.compute_dtype
        xs, eps = self._eng.staged(dt, "x", x32), self._eng.staged(dt, "eps", eps)
        try:
            _lib.check(L.fg_wan_sampler_run(
                self._h, ctypes.byref(sc), ptr(xs), tl_arr, steps, _lib.SAMPLE_TYPES[sample_type], ex, ptr(eps), ctypes.c_uint64(seed), B, F, H, W,
                ptr(ws), ws.numel(), 1 if use_graph else 0, self._stream(dev)))
        finally:
            self._forget_text()  # the loop ends with clear_caches(): the text is forgotten with them
        x.copy_(xs)
        return x

    # ---- the guided teacher sampler as one library call ---------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, noise: torch.Tensor, condition: Any = None, neg_condition: Any = None, guidance_scale: Optional[float] = 5.0,
               sample_steps: int = 50, shift: float = 5.0, context_noise: float = 0, solver: str = "unipc",
               eps: Optional[torch.Tensor] = None, seed: Optional[int] = None, use_graph: bool = True, **kwargs) -> torch.Tensor:
        """`CausalWan.sample` (fastgen/networks/Wan/network_causal.py:1186-1295): autoregressive sampling of the teacher with
        classifier-free guidance over `fg_wan_guided_sampler_run`.  The latents are `noise` itself [B, C, F, H, W], overwritten chunk by
        chunk and returned.  Per chunk and solver step the conditional and the unconditional flow come from ONE network call on the
        stacked batch [x; x] against [condition; neg_condition] (the reference makes two calls under the cache tags "pos" / "neg"; the
        stacked batch keeps both tags' keys / values as rows [0, B) and [B, 2 B) of the tag-"pos" cache set, which holds 2 B rows
        meanwhile), then `v = v_uncond + guidance_scale * (v_cond - v_uncond)` and the solver step are one elementwise pass.  Guided only
        when both guidance_scale and neg_condition are given (the reference would fail on guidance_scale without neg_condition); else
        the loop runs at batch B.

        PARITY UNPINNED: the reference steps diffusers' UniPCMultistepScheduler; solver "unipc" (the default) restates it from the paper
        and "euler" is the plain flow-ODE step (Wan/solvers.py says what differs).  The network sees t = floor(1000 sigma_i) / 1000 where
        diffusers keeps the integer timestep int64(1000 sigma_i) and the reference divides it by 1000 - the same number, unpinned too.
        context_noise > 0: the cache-fill call sees the chunk re-noised with eps ([B, C, F, H, W], injected) or with device draws of
        `seed`.  sample_steps is not bound by the student loops' 64."""
        assert self.schedule_type == "rf", f"{self.schedule_type} is not supported"
        if kwargs:
            raise TypeError(f"unexpected sample kwargs: {sorted(kwargs)}")
        if self.net_pred_type != "flow":
            raise NotImplementedError(f"sample() needs a flow-predicting network, got net_pred_type {self.net_pred_type!r}")
        steps, cn = int(sample_steps), float(context_noise or 0.0)
        text, guided, _, sc, t_arr, table_arr = self._guided_plan(condition, neg_condition, guidance_scale, steps, shift, solver, noise.device,
                                                                  clamp=False, context_noise=cn)
        L = _lib.lib()
        B, F, H, W, dev, ws = self._setup(noise, "noise", L.fg_wan_guided_sampler_workspace_bytes, steps, int(guided),
                                          bad=f"bad video shape or step count: {{}}, {steps} steps")
        self._select_tag("pos")
        self._text_slot.forget()  # (a fresh `text` tensor: embedded for this call)
        self._set_text(text, text.shape[0], dev, ws)
        x32 = noise if (noise.dtype == torch.float32 and noise.is_contiguous()) else noise.to(torch.float32).contiguous()
        if eps is not None:
            eps = eps.to(device=dev, dtype=torch.float32).contiguous()
            if eps.numel() != (x32.numel() if cn > 0 else 0):
                raise ValueError("eps must hold one noise video shaped like noise (context_noise > 0 only)")
        if seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item())
        dt = self._cfg.compute_dtype  # (staging tensors as in student_sample)
        xs, eps = self._eng.staged(dt, "x", x32), self._eng.staged(dt, "eps", eps)
        try:
            _lib.check(L.fg_wan_guided_sampler_run(
                self._h, ctypes.byref(sc), ptr(xs), t_arr, table_arr, steps, ptr(eps), ctypes.c_uint64(seed), B, F, H, W, ptr(ws), ws.numel(),
                1 if use_graph else 0, self._stream(dev)))
        finally:
            self._forget_text()  # the loop ends with clear_caches(): the text is forgotten with them
        noise.copy_(xs)
        return noise
