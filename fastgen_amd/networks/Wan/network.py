"""`Wan` drop-in for the reference's `fastgen.networks.Wan.network.Wan`: the bidirectional video DiT - the network of the DMD2 /
f-distill / LADD few-step WanT2V students (`FastGenModel.generator_fn`), of the MeanFlow student (`r_timestep=True`,
`MeanFlowModel.generator_fn`) and the teacher of all of them (`sample`: UniPC with classifier-free guidance) - backed by
libfastgen_amd.so (`fg_wan_create_ex`, `fg_wan_forward_full`, `fg_wan_full_sampler_run`, `fg_wan_full_guided_sampler_run`).  Every frame
attends to every frame: the engine's all-frames path with one chunk, no self-attention cache, any frame count the RoPE table holds.

As for `CausalWan` (network_causal.py) the fields of the hub config are constructor keywords (defaults = Wan2.1-T2V-1.3B) and the
parameters carry the reference's state-dict keys.  PARITY UNPINNED: the arithmetic lives in un-vendored diffusers (oracle/wan_ref.py
restates it, tests/wan_full_ref.py composes this network from it); the six `transformer.r_embedder.*` keys of `r_timestep=True` and
their order behind `transformer.logvar_linear.*` are read from `init_embedder` (Wan/network.py:799-834), not recorded from a run; the
solver of `sample` restates diffusers' UniPC (Wan/solvers.py).

`expand_timesteps=True` (Wan2.2 TI2V-5B as a text-to-video network: 24 heads, 48 channels, ffn 14336) is accepted and changes nothing:
the reference then hands the embedder one timestep per token, `mask * t` with a mask of ones (Wan/network.py:904-917) - every token of
a sample sees t, which is what the engine's per-frame rows hold already.

Raises (never falls back): autograd, feature taps, logvar, `norm_temb`, `encoder_depth`, timesteps given per token by the caller, image
conditioning (a condition dict: that is `fastgen_amd.networks.WanI2V.network.WanI2V`), skip-layer guidance inside `sample()`
(`forward(skip_layers=...)` serves it), any device but a HIP GPU.
`compute_dtype`: as on `CausalWan` (None / "bf16" / "fp8")."""
from __future__ import annotations

import ctypes
from typing import Any, List, Optional, Set

import torch

from fastgen_amd import _lib
from fastgen_amd.networks import _engine
from fastgen_amd.networks._engine import ptr
from fastgen_amd.networks.Wan._shared import WanEngineNetwork
from fastgen_amd.networks.network import _fused_sample_args
from fastgen_amd.networks.noise_schedule import NET_PRED_TYPES

_T_EMB, _R_EMB = "transformer.condition_embedder.", "transformer.r_embedder."


class Wan(WanEngineNetwork):
    def __init__(self, num_attention_heads: int = 12, attention_head_dim: int = 128, in_channels: int = 16, out_channels: int = 16,
                 text_dim: int = 4096, freq_dim: int = 256, ffn_dim: int = 8960, num_layers: int = 30, eps: float = 1e-6,
                 rope_max_seq_len: int = 1024, r_timestep: bool = False, time_cond_type: str = "diff", r_embedder_init: str = "pretrained",
                 net_pred_type: str = "flow", schedule_type: str = "rf", enable_logvar_linear: bool = True, *,
                 compute_dtype: Optional[str] = None, expand_timesteps: bool = False, **model_kwargs):
        self._check_compute_dtype(compute_dtype, ffn_dim, "bidirectional video DiT")
        self.expand_timesteps = bool(expand_timesteps)  # (see the module docstring: the rows are per frame and the mask is ones)
        self._pop_reference_knobs(model_kwargs, keep=("r_embedder_init", "time_cond_type"))
        if model_kwargs.pop("use_wan_official_sinusoidal", False):
            raise NotImplementedError("use_wan_official_sinusoidal=True is not implemented")
        if time_cond_type not in ("diff", "abs"):
            raise ValueError(f"Invalid time condition: {time_cond_type}")  # (the reference's message, Wan/network.py:337)
        if r_embedder_init not in ("pretrained", "zero", "random"):
            raise ValueError(f"Invalid embedder_init: {r_embedder_init}")  # (:833)
        super().__init__(net_pred_type=net_pred_type, schedule_type=schedule_type, **model_kwargs)
        self.r_timestep, self.time_cond_type, self.r_embedder_init = bool(r_timestep), time_cond_type, r_embedder_init
        ext = _lib.fg_wan_ext_config()
        ext.r_timestep, ext.time_cond_diff = int(self.r_timestep), int(time_cond_type == "diff")
        first = {}  # the first embedder's initial values: the r_embedder starts as its deep copy (:800)

        def init_value(name, shape, g):
            if not name.startswith(_R_EMB):
                v = first[name] = self._init_value(name, shape, g)
                return v
            return first[_T_EMB + name[len(_R_EMB):]].clone()

        # (chunk_size / total_num_frames: the causal calls' business; this module makes none of them)
        self._build_engine(num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim, in_channels=in_channels,
                           out_channels=out_channels, text_dim=text_dim, freq_dim=freq_dim, ffn_dim=ffn_dim, num_layers=num_layers, eps=eps,
                           rope_max_seq_len=rope_max_seq_len, chunk_size=1, total_num_frames=1, compute_dtype=compute_dtype,
                           enable_logvar_linear=enable_logvar_linear, ext=ext, init_value=init_value)
        self.num_layers = num_layers
        if self.r_timestep:
            self.init_r_embedder(r_embedder_init)

    @torch.no_grad()
    def init_r_embedder(self, how: str, generator: Optional[torch.Generator] = None) -> None:
        """`Wan.init_embedder` (Wan/network.py:799-834) on the r_embedder as it stands (after construction, or after a checkpoint
        without it was loaded with strict=False): "pretrained" - the condition_embedder's time_embedder / time_proj values; "zero" -
        every parameter zero; "random" - xavier-uniform weights with zero biases, the time_embedder's weights normal(0, 0.02), then
        time_embedder.linear_2 and time_proj zero: remb and r_timestep_proj start at zero."""
        if not self.r_timestep:
            raise ValueError("this network has no r_embedder (r_timestep=False)")
        if how not in ("pretrained", "zero", "random"):
            raise ValueError(f"Invalid embedder_init: {how}")
        params = dict(self.named_parameters())
        g = generator or torch.Generator().manual_seed(0)
        for name, p in params.items():
            if not name.startswith(_R_EMB):
                continue
            if how == "pretrained":
                p.copy_(params[_T_EMB + name[len(_R_EMB):]])
            elif how == "zero" or name.endswith(".bias") or "linear_2" in name or "time_proj" in name:
                p.zero_()
            else:  # time_embedder.linear_1.weight, the one parameter that stays random
                p.copy_((torch.randn(p.shape, generator=g) * 0.02).to(p.device))

    # ---- the condition beside the text: what a dict-conditioned subclass (WanI2V, VACEWan) states ------------------------------------
    @staticmethod
    def _split_condition(condition: Any, what: str = "condition"):
        """`condition` as (the text, the rest: a tuple of what `_set_rest` takes).  A subclass asserts its dict's keys here."""
        return condition, ()

    def _set_rest(self, rest, B: int, F: int, H: int, W: int, dev) -> None:
        """Hand the rest of the condition to the handle for a call at batch B on an [F, H, W] video (after `_bind`: packing forgets it)."""

    def _sample_rest(self, rest, neg_rest, dev):
        """The rest of the condition for `sample`: stacked [condition; neg_condition] when guided (`neg_rest` is not None)."""
        return rest

    def _prepare(self, x: torch.Tensor, what: str, *rest, stack: int = 1) -> None:
        """The rest of the condition into the handle as a call on `x` (`what` in the messages) at `stack` times its batch would set it."""
        _engine.require_gpu(x)
        B, F, H, W = self._check_video(x, what)
        self._bind(x.device)  # (first: packing would invalidate what is set below)
        self._set_rest(rest, B * stack, F, H, W, x.device)

    # ---- one network call ---------------------------------------------------------------------------------------------------
    def forward(self, x_t: torch.Tensor, t: torch.Tensor, condition: Optional[Any] = None, r: Optional[torch.Tensor] = None,
                return_features_early: bool = False, feature_indices: Optional[Set[int]] = None, return_logvar: bool = False,
                unpatchify_features: bool = True, fwd_pred_type: Optional[str] = None, skip_layers: Optional[List[int]] = None,
                **fwd_kwargs):
        text, rest = self._split_condition(condition)
        if feature_indices or return_features_early or return_logvar:
            raise NotImplementedError("feature taps / logvar are not implemented for the bidirectional video DiT path")
        if fwd_kwargs:
            raise TypeError(f"unexpected forward kwargs: {sorted(fwd_kwargs)}")
        if r is not None and not self.r_timestep:
            raise ValueError("r_timestep provided but no r_embedder is present")  # (the reference's, Wan/network.py:356)
        if fwd_pred_type is None:
            fwd_pred_type = self.net_pred_type
        else:
            assert fwd_pred_type in NET_PRED_TYPES, f"{fwd_pred_type} is not supported as fwd_pred_type"
        t_in = torch.atleast_1d(t.detach()).to(x_t.device)
        if t_in.ndim != 1:
            raise NotImplementedError(f"t must be [B] (timesteps given per token, [B, seq_len], are not implemented: expand_timesteps "
                                      f"expands a [B] t inside the network), got {tuple(t_in.shape)}")
        self._no_autograd(x_t)
        text = self._text(text)
        L = _lib.lib()
        B, F, H, W, dev, ws = self._setup(x_t, "x_t", L.fg_wan_full_workspace_bytes)
        skip = sorted(set(int(i) for i in skip_layers)) if skip_layers else []
        if skip and (skip[0] < 0 or skip[-1] >= self.num_layers):
            raise ValueError(f"skip_layers must be block indices in [0, {self.num_layers}), got {list(skip_layers)}")

        def rows(name, v):  # [B] in the schedule's units -> one embedder row per frame
            return self._frame_rows(self.noise_scheduler.rescale_t(_engine.per_sample(name, v, B, dev)), B, F)

        ts = rows("t", t_in)
        rs = rows("r", r) if r is not None else None
        self._set_rest(rest, B, F, H, W, dev)
        self._set_text(text, B, dev, ws)
        x32 = x_t.detach().to(torch.float32).contiguous()
        out = torch.empty_like(x32)
        _lib.check(L.fg_wan_forward_full(self._h, ptr(x32), ptr(ts), ptr(rs), ptr(out), B, F, H, W,
                                         (ctypes.c_int * len(skip))(*skip) if skip else None, len(skip), ptr(ws), ws.numel(), self._stream(dev)))
        return self.noise_scheduler.convert_model_output(x_t, out.to(x_t.dtype), _engine.per_sample("t", t_in, B, dev),
                                                         src_pred_type=self.net_pred_type, target_pred_type=fwd_pred_type)

    @torch.no_grad()
    def jvp(self, x_t: torch.Tensor, t: torch.Tensor, v_x: torch.Tensor, v_t: Optional[torch.Tensor] = None, condition: Optional[Any] = None,
            r: Optional[torch.Tensor] = None, v_r: Optional[torch.Tensor] = None, fwd_pred_type: Optional[str] = None):
        """(output, directional derivative) of `forward(x_t, t, condition=condition, r=r)` along (v_x, v_t, v_r) - what
        `torch.func.jvp(net_wrapper, (x_t, t, r), tangents)` would return in MeanFlowModel._jvp (mean_flow.py:240-250; the reference
        itself falls back to a finite difference for this network) - as one library call (`fg_wan_jvp`: a bf16 tangent stream beside
        the bf16 primal stream).  Forward-only and stateless: no graph is built.  `forward()`'s preparation of (t, r) - `rescale_t`,
        one row per frame - is applied here, and its derivative to (v_t, v_r); under time_cond_type "diff" the engine forms t - r and
        v_t - v_r.  Raises NotImplementedError (never falls back): compute_dtype "fp8", the image-to-video and VACE subclasses, another
        prediction type than the network's own, CPU tensors."""
        L = _lib.lib()
        # the handle's kind first (an image-to-video or VACE subclass, the fp8 mode): its refusal comes before any look at the shapes,
        # which those networks define differently
        if L.fg_wan_jvp_workspace_bytes(self._h, 1, 1, 2, 2) == 0:
            raise NotImplementedError(f"fastgen_amd.{type(self).__name__}.jvp: this network has no forward-mode derivative (a plain "
                                      f"text-to-video Wan in the bf16 compute mode has one)")
        if fwd_pred_type is not None and fwd_pred_type != self.net_pred_type:
            raise NotImplementedError("jvp is provided for the network's own prediction type")
        if r is None and self.r_timestep:
            raise ValueError("this network was built with r_timestep=True: jvp() needs r")
        if r is not None and not self.r_timestep:
            raise ValueError("r_timestep provided but no r_embedder is present")
        if not x_t.is_cuda:
            raise NotImplementedError("fastgen_amd.Wan.jvp runs on a HIP GPU only (no CPU path)")

        def need(h, B, F, H, W):  # also the text embedding's scratch (the query at the smallest video is that scratch)
            n = L.fg_wan_jvp_workspace_bytes(h, B, F, H, W)
            return n and max(n, L.fg_wan_full_workspace_bytes(h, B, 1, 2, 2))

        # a workspace of its own: forward()'s is neither used nor regrown here, it stays where a captured sampler saw it
        B, F, H, W, dev, ws = self._setup(x_t, "x_t", need, key=("jvp", self._cfg.compute_dtype))
        if v_x.shape != x_t.shape:
            raise ValueError(f"v_x must be shaped like x_t {tuple(x_t.shape)}, got {tuple(v_x.shape)}")
        condition = self._text(condition)
        sch = self.noise_scheduler

        def tangent(name, v):  # the derivative of rescale_t, a multiplication by num_steps or 1
            if v is None:
                return None
            return self._frame_rows(sch._rescale(_engine.per_sample(name, v, B, dev).to(torch.float32)), B, F)

        ts = self._frame_rows(sch.rescale_t(_engine.per_sample("t", torch.atleast_1d(t.detach()).to(dev), B, dev)), B, F)
        rs = self._frame_rows(sch.rescale_t(_engine.per_sample("r", r, B, dev)), B, F) if r is not None else None
        vts, vrs = tangent("v_t", v_t), (tangent("v_r", v_r) if r is not None else None)
        self._set_text(condition, B, dev, ws)
        x32 = x_t.detach().to(torch.float32).contiguous()
        vx = v_x.detach().to(device=dev, dtype=torch.float32).contiguous()
        out, jv = torch.empty_like(x32), torch.empty_like(x32)
        _lib.check(L.fg_wan_jvp(self._h, ptr(x32), ptr(ts), ptr(rs), ptr(vx), ptr(vts), ptr(vrs), ptr(out), ptr(jv), B, F, H, W, None, 0, ptr(ws),
                                ws.numel(), self._stream(dev)))
        return out.to(x_t.dtype), jv.to(x_t.dtype)

    # ---- the student loops over the whole video as one library call --------------------------------------------------------------
    def supports_fused_loop(self, kind: str) -> bool:
        """Which loops `fg_wan_full_sampler_run` restates for this network: 'x0' (FastGenModel._student_sample_loop; flow- or
        x0-predicting network) and 'meanflow' (MeanFlowModel._student_sample_loop: flow-predicting network with the r_embedder)."""
        if self.net_pred_type not in ("flow", "x0") or self.schedule_type not in ("rf", "rectified_flow", "edm"):
            return False
        return kind == "x0" or (kind == "meanflow" and self.r_timestep and self.net_pred_type == "flow")

    def few_step_sample(self, noise: torch.Tensor, condition: Any, t_list, sample_type: str = "sde", eps: Optional[torch.Tensor] = None,
                        seed: Optional[int] = None, use_graph: bool = True, loop: str = "x0") -> torch.Tensor:
        """The whole sampling loop over the whole video as ONE `fg_wan_full_sampler_run` call / one hipGraph replay: latents = noise *
        sigma(t_list[0]), then per step the network call and the schedule arithmetic of `loop` ('x0' | 'meanflow').  'sde' re-noises with
        `eps` ([steps - 1, B, C, F, H, W], injected) or device normals drawn from `seed`."""
        text, rest = self._split_condition(condition)
        self._no_autograd()
        if not self.supports_fused_loop(loop):
            raise NotImplementedError(f"the fused sampler has no loop {loop!r} for net_pred_type={self.net_pred_type!r}, "
                                      f"r_timestep={self.r_timestep}, schedule_type={self.schedule_type!r}")
        n32, steps, tl_arr, eps, seed = _fused_sample_args(noise, t_list, sample_type, eps, seed)
        text = self._text(text)
        L = _lib.lib()
        B, F, H, W, dev, ws = self._setup(noise, "noise", L.fg_wan_full_sampler_workspace_bytes)
        self._set_rest(rest, B, F, H, W, dev)
        self._set_text(text, B, dev, ws)
        sc = self._sampler_config()
        # every device pointer of the call is in the graph's key: the call runs on the handle's staging tensors, so that a second call
        # with the same shapes replays the graph whatever tensors the caller passes
        dt, st = self._cfg.compute_dtype, self._eng.staged
        n32, eps, out = st(dt, "noise", n32), st(dt, "eps", eps), st(dt, "out", like=n32)
        _lib.check(L.fg_wan_full_sampler_run(
            self._h, ctypes.byref(sc), ptr(n32), tl_arr, steps, _lib.SAMPLE_TYPES[sample_type], _lib.LOOP_KINDS[loop], ptr(eps),
            ctypes.c_uint64(seed), ptr(out), B, F, H, W, ptr(ws), ws.numel(), 1 if use_graph else 0, self._stream(dev)))
        return out.to(noise.dtype, copy=True)  # the caller's own tensor

    # ---- the guided teacher sampler as one library call ------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, noise: torch.Tensor, condition: Any = None, neg_condition: Any = None, guidance_scale: Optional[float] = 5.0,
               num_steps: int = 50, shift: float = 5.0, skip_layers: Optional[List[int]] = None, skip_layers_start_percent: float = 0.0,
               solver: str = "unipc", use_graph: bool = True, **kwargs) -> torch.Tensor:
        """`Wan.sample` (fastgen/networks/Wan/network.py:919-988) over `fg_wan_full_guided_sampler_run`: latents = noise * sigma(t_0),
        then per solver step the conditional and the unconditional flow from ONE network call on the stacked batch [x; x] against
        [condition; neg_condition], `v = v_uncond + guidance_scale * (v_cond - v_uncond)` and the solver step as one elementwise pass;
        one hipGraph for the video.  Guided only when both guidance_scale and neg_condition are given (the reference would fail on
        guidance_scale without neg_condition); else the loop runs at batch B.  Returns a new tensor; `noise` is left as it is.

        PARITY UNPINNED: solver "unipc" (the default) restates diffusers' UniPCMultistepScheduler and "euler" is the plain flow-ODE
        step (Wan/solvers.py).  The network sees t_i = min(floor(1000 sigma_i) / 1000, max_t): the scheduler's integer timestep over
        num_train_timesteps, clamped as the reference clamps it (:958-961)."""
        text, rest = self._split_condition(condition)
        assert self.schedule_type == "rf", f"{self.schedule_type} is not supported"
        if kwargs:
            raise TypeError(f"unexpected sample kwargs: {sorted(kwargs)}")
        if skip_layers:
            raise NotImplementedError("skip_layers in sample() (skip-layer guidance on the unconditional call) is not implemented; "
                                      "forward(skip_layers=...) serves a loop of separate calls")
        if self.net_pred_type != "flow":
            raise NotImplementedError(f"sample() needs a flow-predicting network, got net_pred_type {self.net_pred_type!r}")
        neg_text, neg_rest = None, None
        if guidance_scale is not None and neg_condition is not None:
            neg_text, neg_rest = self._split_condition(neg_condition, "neg_condition")
        rest = self._sample_rest(rest, neg_rest, noise.device)
        steps = int(num_steps)
        text, guided, t_net, sc, t_arr, table_arr = self._guided_plan(text, neg_text, guidance_scale, steps, shift, solver, noise.device, clamp=True)
        L = _lib.lib()
        B, F, H, W, dev, ws = self._setup(noise, "noise", L.fg_wan_full_guided_sampler_workspace_bytes, steps, int(guided),
                                          bad=f"bad video shape or step count: {{}}, {steps} steps")
        self._set_rest(rest, B * (2 if guided else 1), F, H, W, dev)
        self._text_slot.forget()  # (a fresh `text` tensor when guided: embedded for this call)
        self._set_text(text, text.shape[0], dev, ws)
        latents = self.noise_scheduler.latents(noise=noise.to(torch.float32), t_init=t_net[0].to(dev))  # (:952-954)
        xs = self._eng.staged(self._cfg.compute_dtype, "x", latents.contiguous())  # (staging tensor as in few_step_sample)
        try:
            _lib.check(L.fg_wan_full_guided_sampler_run(self._h, ctypes.byref(sc), ptr(xs), t_arr, table_arr, steps, B, F, H, W, ptr(ws), ws.numel(),
                                                        1 if use_graph else 0, self._stream(dev)))
        finally:
            if guided:
                self._forget_text()  # the handle holds the stacked condition: the next call sets its own
        return xs.to(noise.dtype, copy=True)
