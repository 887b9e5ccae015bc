"""`EDM2Precond` drop-in for the reference's `fastgen.networks.EDM2.network.EDM2Precond` (the magnitude-preserving EDM2 U-Net of the
ImageNet-64 consistency-model recipes, configs/net.py EDM2_IN64_*_Config), backed by libfastgen_amd.so (the fg_edm2_* entry points).

Select it by pointing a config's `net._target_` at `fastgen_amd.networks.EDM2.network.EDM2Precond`.  Kept identical to the reference:
  * constructor kwargs (those of EDM2Precond, EMD2UNet and Block), `.noise_scheduler`, `.net_pred_type`, `.label_dim`, `sample()`,
    `forced_weight_normalization()`;
  * `state_dict()`: the reference's names, order and shapes, the four Fourier buffers included, so a reference checkpoint loads with
    strict=True;
  * `forward(x_t, t, condition, r, return_features_early, feature_indices, return_logvar, fwd_pred_type)` in eval mode.
Parameters hold the raw (un-normalised) weights, as in the reference; the library normalises and packs them whenever a parameter's
storage or version changes.  `supports_fused_loop("x0")` / `few_step_sample` let `FastGenModel.generator_fn` run the whole student
loop as one library call (one hipGraph replay).

Forward, sampling and `jvp` (the forward-mode derivative sCM's TrigFlowPrecond.jvp takes, fg_edm2_jvp), in the 'bf16x3' (default for
fp32 tensors) and 'bf16' (under bf16 autocast) compute modes.  Autograd, train() mode with dropout, fully_shard, feature taps,
r_timestep, the positional embedding, exact fp32, channels_per_head != 64 and resample_filter != [1, 1] raise NotImplementedError.
There is no CPU path (`jvp` on CPU tensors raises NotImplementedError too).
"""
from __future__ import annotations

import math
import os
from typing import Optional, Set

import numpy as np
import torch
import torch.nn as nn

from fastgen_amd import _lib
from fastgen_amd.networks import _engine
from fastgen_amd.networks._engine import _Node, ptr, stream
from fastgen_amd.networks.network import FastGenNetwork, _edm_euler_sample, _fused_sample_args
from fastgen_amd.networks.noise_schedule import NET_PRED_TYPES

DEFAULT_FP32_MODE = "bf16x3"  # as fastgen_amd.networks.EDM.network


def _mp_weight(w: torch.Tensor, gain=1.0) -> torch.Tensor:
    """MPConv's forward weight: normalize (eps 1e-4), then gain / sqrt(fan_in)."""
    w = w.to(torch.float32)
    fan_in = w[0].numel()
    norm = torch.linalg.vector_norm(w, dim=list(range(1, w.ndim)), keepdim=True) / math.sqrt(fan_in)
    return w / (1e-4 + norm) * (gain / math.sqrt(fan_in))


class EDM2Precond(FastGenNetwork):
    def __init__(
        self,
        img_resolution,
        img_channels,
        label_dim,
        sigma_data=0.5,
        sigma_shift=0.0,
        logvar_channels=128,
        drop_precond=None,
        net_pred_type="x0",
        schedule_type="edm",
        compute_dtype: Optional[str] = None,  # extension: "bf16x3" | "bf16" | None (= follow torch.autocast)
        **model_kwargs,
    ):
        super().__init__(net_pred_type=net_pred_type, schedule_type=schedule_type, **model_kwargs)
        if drop_precond is not None and drop_precond not in ["input", "output", "both"]:
            raise ValueError(f"drop_precond must be one of 'input', 'output', 'both', or None, got {drop_precond}")
        mk = dict(model_kwargs)
        if mk.get("embedding_type", "mp_fourier") not in ("mp_fourier", "positional"):
            raise ValueError(f"embedding_type must be 'mp_fourier' or 'positional', got {mk['embedding_type']!r}")
        if mk.get("embedding_type", "mp_fourier") != "mp_fourier":
            raise NotImplementedError("embedding_type='positional' is not implemented for EDM2 by the fused MI355X path")
        if mk.get("r_timestep", False):
            raise NotImplementedError("r_timestep=True is not implemented for EDM2 by the fused MI355X path")
        if mk.get("channels_per_head", 64) != 64:
            raise NotImplementedError("channels_per_head other than 64 is not implemented for EDM2")
        if list(mk.get("resample_filter", [1, 1])) != [1, 1]:
            raise NotImplementedError("resample_filter other than [1, 1] is not implemented for EDM2")
        if schedule_type != "edm":
            raise NotImplementedError(f"schedule_type={schedule_type!r} is not implemented for EDM2 by the fused MI355X path")
        self.compute_dtype = compute_dtype or os.environ.get("FASTGEN_AMD_COMPUTE_DTYPE") or None
        if self.compute_dtype == "fp32":
            raise NotImplementedError("EDM2 runs in the 'bf16x3' (default) and 'bf16' compute modes, not in exact fp32")
        if self.compute_dtype == "fp8":
            raise ValueError("compute_dtype='fp8' is implemented for the DiT only (EDM2Precond: 'bf16x3', 'bf16' or None)")
        if self.compute_dtype not in (None, "bf16x3", "bf16"):
            raise ValueError(f"compute_dtype must be 'bf16x3', 'bf16' or None, got {self.compute_dtype!r}")
        self.img_resolution = img_resolution
        self.img_channels = img_channels
        self.label_dim = label_dim
        self.sigma_data = sigma_data
        self.sigma_shift = sigma_shift
        self.drop_precond = drop_precond
        self.r_timestep = False
        self.dropout = float(mk.get("dropout", 0) or 0)
        bandwidth = float(mk.get("mp_fourier_bandwidth", 1.0))

        mult = list(mk.get("channel_mult", [1, 2, 3, 4]))
        attn = list(mk.get("attn_resolutions", [16, 8]))
        if len(mult) > _lib.FG_MAX_LEVELS or len(attn) > _lib.FG_MAX_LEVELS:
            raise ValueError("too many resolution levels")
        cfg = _lib.fg_edm2_config()
        cfg.img_resolution, cfg.img_channels, cfg.label_dim = img_resolution, img_channels, label_dim
        cfg.model_channels = mk.get("model_channels", 192)
        cfg.num_levels = len(mult)
        for i, m in enumerate(mult):
            cfg.channel_mult[i] = m
        cfg.channel_mult_noise = mk.get("channel_mult_noise") or 0
        cfg.channel_mult_emb = mk.get("channel_mult_emb") or 0
        cfg.num_blocks = mk.get("num_blocks", 3)
        cfg.num_attn_resolutions = len(attn)
        for i, a in enumerate(attn):
            cfg.attn_resolutions[i] = a
        cfg.label_balance = mk.get("label_balance", 0.5)
        cfg.concat_balance = mk.get("concat_balance", 0.5)
        cfg.res_balance = mk.get("res_balance", 0.3)
        cfg.attn_balance = mk.get("attn_balance", 0.3)
        clip = mk.get("clip_act", 256)
        cfg.clip_act = float(clip) if clip is not None else 0.0
        cfg.sigma_data, cfg.sigma_shift = float(sigma_data), float(sigma_shift)
        cfg.drop_precond = {None: 0, "input": _lib.FG_DROP_PRECOND_INPUT, "output": _lib.FG_DROP_PRECOND_OUTPUT,
                            "both": _lib.FG_DROP_PRECOND_INPUT | _lib.FG_DROP_PRECOND_OUTPUT}[drop_precond]
        self._cfg = cfg
        self._eng = _engine.Handles("edm2", cfg)

        # the tree of the reference's key paths; names / shapes / order from the library's plan (its state_dict() order)
        self.unet = _Node()

        def register(node, leaf, full, shp):
            if leaf == "freqs":
                node.register_buffer(leaf, 2 * np.pi * torch.randn(shp) * bandwidth)
            elif leaf == "phases":
                node.register_buffer(leaf, 2 * np.pi * torch.rand(shp))
            elif leaf in ("emb_gain", "out_gain"):
                node.register_parameter(leaf, nn.Parameter(torch.zeros(shp)))
            else:
                node.register_parameter(leaf, nn.Parameter(torch.randn(shp)))

        self._names, self._leafs = _engine.build_tree(self, "edm2", self._eng.get(_lib.FG_DTYPE_BF16X3), register)
        # the logvar head: host-side torch (MPFourier(logvar_channels) + MPConv(logvar_channels, 1))
        self.logvar_fourier = _Node()
        self.logvar_fourier.register_buffer("freqs", 2 * np.pi * torch.randn(logvar_channels) * bandwidth)
        self.logvar_fourier.register_buffer("phases", 2 * np.pi * torch.rand(logvar_channels))
        self.logvar_linear = _Node()
        self.logvar_linear.register_parameter("weight", nn.Parameter(torch.randn(1, logvar_channels)))

    # ------------------------------------------------------------------------------------------------
    def _make_engine(self, dtype: int):
        return self._eng.create(dtype)

    def _select_dtype(self) -> int:
        mode = _engine.compute_mode(self.compute_dtype, DEFAULT_FP32_MODE)
        if mode == "fp32":
            raise NotImplementedError("EDM2 runs in the 'bf16x3' and 'bf16' compute modes, not in exact fp32")
        return _lib.DTYPE_NAMES[mode]

    def _engine(self, device: torch.device):
        """Engine of the active compute mode with the module's current weights bound and packed."""
        dt = self._select_dtype()
        h = self._eng.get(dt)
        # the parameters and the Fourier buffers in engine order, straight from the leaf modules' dicts
        ts = [leaf._parameters[n] if n in leaf._parameters else leaf._buffers[n] for leaf, n in self._leafs]
        self._eng.bind_in_place(dt, self._names, ts, device)
        _lib.check(_lib.lib().fg_edm2_set_training(h, int(self.training)))
        return dt, h

    def _workspace(self, dt: int, h, batch: int, device) -> torch.Tensor:
        return self._eng.workspace(dt, _lib.lib().fg_edm2_workspace_bytes(h, batch), device)

    _stream = staticmethod(stream)

    def _refuse_training(self, x_t: Optional[torch.Tensor] = None):
        if torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters()) or (x_t is not None and x_t.requires_grad)):
            raise NotImplementedError("autograd through EDM2Precond is not implemented by the fused MI355X path (forward and sampling "
                                      "only): call it under torch.no_grad() / torch.inference_mode()")
        if self.training and self.dropout > 0:
            raise NotImplementedError("train() mode with dropout > 0 is not implemented for EDM2 by the fused MI355X path")

    def _labels(self, condition, batch: int, device) -> Optional[torch.Tensor]:
        return _engine.class_labels(condition, self.label_dim, batch, device)  # (None: emb_label(zeros) = 0, as the reference's zero labels give)

    # ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forced_weight_normalization(self):
        """normalize() every MPConv weight in place (the reference's normalize_weights); the engine repacks on the next call."""
        for n, p in self.named_parameters():
            if n.endswith(".weight"):
                fan_in = p[0].numel()
                norm = torch.linalg.vector_norm(p.to(torch.float32), dim=list(range(1, p.ndim)), keepdim=True) / math.sqrt(fan_in)
                p.copy_((p / (1e-4 + norm).to(p.dtype)))

    def reset_parameters(self):
        raise NotImplementedError("reset_parameters (FSDP meta-device initialisation) is not implemented for EDM2")

    def fully_shard(self, **kwargs):
        raise NotImplementedError("fully_shard is not implemented for EDM2 by the fused MI355X path (forward and sampling only)")

    @torch.no_grad()
    def jvp(self, x_t: torch.Tensor, t: torch.Tensor, v_x: torch.Tensor, v_t: Optional[torch.Tensor] = None,
            condition: Optional[torch.Tensor] = None, r: Optional[torch.Tensor] = None, v_r: Optional[torch.Tensor] = None,
            fwd_pred_type: Optional[str] = None):
        """(output, directional derivative) of `forward(x_t, t, condition=condition)` along (v_x, v_t) - what
        `torch.func.jvp(net_wrapper, (x_t, t), tangents)` returns in sCM's TrigFlowPrecond.jvp (SCMModel._jvp) - as one library call
        (fg_edm2_jvp): the primal and the tangent stream run block by block in the active compute mode, and the output is forward()'s
        bit for bit.  The contract of EDMPrecond.jvp: no graph is built (the reference detaches the result too)."""
        if fwd_pred_type is not None and fwd_pred_type != self.net_pred_type:
            raise NotImplementedError("jvp is provided for the network's own prediction type")
        if r is not None or v_r is not None:
            raise ValueError("r / v_r provided, but EDM2 has no r_timestep")
        self._refuse_training()
        self._select_dtype()
        if x_t.device.type != "cuda":  # no CPU path: not implemented, like the module's other refusals
            raise NotImplementedError("EDM2Precond.jvp runs on a HIP GPU only (there is no CPU path); got a tensor on " + str(x_t.device))
        R, C = self.img_resolution, self.img_channels
        if x_t.dim() != 4 or tuple(x_t.shape[1:]) != (C, R, R):
            raise ValueError(f"x_t must be [B,{C},{R},{R}], got {tuple(x_t.shape)}")
        if v_x.shape != x_t.shape:
            raise ValueError(f"v_x must have x_t's shape {tuple(x_t.shape)}, got {tuple(v_x.shape)}")
        B, dev = x_t.shape[0], x_t.device
        x32 = x_t.detach().to(torch.float32).contiguous()
        vx = v_x.detach().to(device=dev, dtype=torch.float32).contiguous()
        t64 = _engine.per_sample("t", t, B, dev, torch.float64)
        vt = None if v_t is None else _engine.per_sample("v_t", v_t, B, dev, torch.float32)
        labels = self._labels(condition, B, dev)
        dt, h = self._engine(dev)
        L = _lib.lib()
        ws = self._eng.workspace(("jvp", dt), L.fg_edm2_jvp_workspace_bytes(h, B), dev)  # its own: forward()'s stays where a captured sampler saw it
        out, jv = torch.empty_like(x32), torch.empty_like(x32)
        _lib.check(L.fg_edm2_jvp(h, ptr(x32), ptr(t64), ptr(labels), ptr(vx), ptr(vt), ptr(out), ptr(jv), B, ptr(ws), ws.numel(),
                                 self._stream(dev)))
        return out.to(x_t.dtype), jv.to(x_t.dtype)

    def _c_noise(self, t64: torch.Tensor) -> torch.Tensor:
        if self.drop_precond in ("input", "both"):
            return t64.to(torch.float32)
        return (t64.clamp(min=self.noise_scheduler.clamp_min).log() / 4).to(torch.float32)

    def _logvar(self, t64: torch.Tensor) -> torch.Tensor:
        """logvar_linear(logvar_fourier(c_noise)) with torch on the module's own parameters."""
        lf = self.logvar_fourier
        y = self._c_noise(t64).ger(lf.freqs.to(device=t64.device, dtype=torch.float32))
        y = (y + lf.phases.to(device=t64.device, dtype=torch.float32)).cos() * np.sqrt(2)
        return (y @ _mp_weight(self.logvar_linear.weight).t()).reshape(-1, 1)

    def forward(
        self,
        x_t: torch.Tensor,
        t: torch.Tensor,
        condition: Optional[torch.Tensor] = None,
        r: Optional[torch.Tensor] = None,
        return_features_early: bool = False,
        feature_indices: Optional[Set[int]] = None,
        return_logvar: bool = False,
        fwd_pred_type: Optional[str] = None,
        **fwd_kwargs,
    ):
        if feature_indices is None:
            feature_indices = {}
        if len(feature_indices):
            raise NotImplementedError("feature_indices / return_features_early are not implemented for EDM2 by the fused MI355X path")
        if return_features_early:
            return []
        if fwd_pred_type is None:
            fwd_pred_type = self.net_pred_type
        else:
            assert fwd_pred_type in NET_PRED_TYPES, f"{fwd_pred_type} is not supported as fwd_pred_type"
        if r is not None:
            raise ValueError("r_noise_labels provided, but r_timestep is not set")
        if fwd_kwargs:
            raise TypeError(f"unexpected forward kwargs: {sorted(fwd_kwargs)}")
        self._refuse_training(x_t)
        self._select_dtype()
        _engine.require_gpu(x_t)
        R, C = self.img_resolution, self.img_channels
        if x_t.dim() != 4 or tuple(x_t.shape[1:]) != (C, R, R):
            raise ValueError(f"x_t must be [B,{C},{R},{R}], got {tuple(x_t.shape)}")
        B, dev = x_t.shape[0], x_t.device
        x32 = x_t.detach().to(torch.float32).contiguous()
        t64 = _engine.per_sample("t", t, B, dev, torch.float64)
        labels = self._labels(condition, B, dev)
        dt, h = self._engine(dev)
        ws = self._workspace(dt, h, B, dev)
        out = torch.empty_like(x32)
        _lib.check(_lib.lib().fg_edm2_forward(h, ptr(x32), ptr(t64), ptr(labels), ptr(out), None, B, ptr(ws), ws.numel(), self._stream(dev)))
        out = out.to(x_t.dtype)
        out = self.noise_scheduler.convert_model_output(x_t, out, t64, src_pred_type=self.net_pred_type, target_pred_type=fwd_pred_type)
        if return_logvar:
            return out, self._logvar(t64)
        return out

    # ------------------------------------------------------------------------------------------------
    def fused_loop(self) -> Optional[str]:
        return "x0" if self.net_pred_type == "x0" else None

    def supports_fused_loop(self, kind: str) -> bool:
        return kind is not None and self.fused_loop() == kind

    def few_step_sample(self, noise: torch.Tensor, condition: Optional[torch.Tensor], t_list, sample_type: str = "sde",
                        eps: Optional[torch.Tensor] = None, seed: Optional[int] = None, use_graph: bool = True,
                        out: Optional[torch.Tensor] = None, loop: Optional[str] = None) -> torch.Tensor:
        """FastGenModel._student_sample_loop (methods/model.py:374-420) as ONE library call / one hipGraph replay; arguments as
        EDMPrecond.few_step_sample (x0 loop only)."""
        self._refuse_training()
        loop = loop or self.fused_loop()
        if loop is None or loop != self.fused_loop():
            raise NotImplementedError(f"the fused sampler has no loop {loop!r} for net_pred_type={self.net_pred_type!r}")
        n32, steps, tl_arr, eps, seed = _fused_sample_args(noise, t_list, sample_type, eps, seed)
        B, dev = noise.shape[0], noise.device
        labels = self._labels(condition, B, dev)
        dt, h = self._engine(dev)
        ws = self._workspace(dt, h, B, dev)
        return _engine.run_x0_sampler(_lib.lib().fg_edm2_sampler_run, self._eng, dt, h, n32, labels, tl_arr, steps, sample_type, loop, eps, seed,
                                      out, B, ws, use_graph, dev)

    def sample(self, noise: torch.Tensor, condition: Optional[torch.Tensor] = None, neg_condition: Optional[torch.Tensor] = None,
               guidance_scale: Optional[float] = 5.0, num_steps: int = 50, **kwargs) -> torch.Tensor:
        """EDM2's deterministic Euler sampler with optional classifier-free guidance, one forward() per step."""
        return _edm_euler_sample(self, noise, condition, neg_condition, guidance_scale, num_steps)
