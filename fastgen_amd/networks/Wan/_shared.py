"""What the two Wan modules (`CausalWan`, network_causal.py; `Wan`, network.py) do alike with their `fg_wan_*` handle: the reference
knobs they take and refuse, the handle and the parameter tree from the library's plan, the initial values, binding, the condition
slots and the text condition, the setup of a call (shape, binding, workspace), the sampler configs, the guided teacher's plan and
`fully_shard`.  What a network does differently - its calls, its caches, its refusals - stays in its own module."""
from __future__ import annotations

import ctypes
import weakref
from typing import Any, Optional

import torch
import torch.nn as nn

from fastgen_amd import _lib
from fastgen_amd.networks import _engine
from fastgen_amd.networks._engine import ptr, stream
from fastgen_amd.networks.network import FastGenNetwork

# reference knobs without meaning here (hub ids, autograd plumbing); a module keeps those it consumes itself (`keep`)
_IGNORED = ("model_id_or_local_path", "load_pretrained", "disable_efficient_attn", "disable_grad_ckpt", "use_fsdp_checkpoint",
            "r_embedder_init", "time_cond_type", "norm_temb", "encoder_depth", "delete_cache_on_clear")


class ConditionSlot:
    """What was last handed to the handle under one name, so that it is handed over once: per tensor the object (a weakref), its
    in-place version (0 for an inference tensor, which has none to read) and its shape - the reference's static cache; a new object on
    recycled storage is handed over again.  A None member (an absent image) matches only None; `extra`: plain values that take part."""

    def __init__(self):
        self._key = None

    @staticmethod
    def _version(t: torch.Tensor) -> int:
        return 0 if t.is_inference() else t._version

    def same(self, *tensors, extra=()) -> bool:
        def is_same(a, t):
            if a is None or t is None:
                return a is None and t is None
            return a[0]() is t and a[1] == self._version(t) and a[2] == t.shape

        k = self._key
        return k is not None and k[1] == tuple(extra) and len(k[0]) == len(tensors) and all(map(is_same, k[0], tensors))

    def remember(self, *tensors, extra=()) -> None:
        self._key = ([None if t is None else (weakref.ref(t), self._version(t), tuple(t.shape)) for t in tensors], tuple(extra))

    def forget(self) -> None:
        self._key = None


class WanEngineNetwork(FastGenNetwork):
    """The module tree and the engine plumbing over one `fg_wan` handle (the compute mode is fixed at construction)."""
    _NAME = "Wan"  # (in the refusals' texts)
    _SLOTS = ("text",)  # the conditions on the handle that packing invalidates, one `ConditionSlot` each

    @staticmethod
    def _check_compute_dtype(compute_dtype: Optional[str], ffn_dim: int, what: str) -> None:
        if compute_dtype not in (None, "bf16", "fp8"):
            raise ValueError(f"compute_dtype must be None, 'bf16' or 'fp8' for the {what}, got {compute_dtype!r}")
        if compute_dtype == "fp8" and ffn_dim % 128:
            raise ValueError(f"compute_dtype='fp8' needs ffn_dim to be a multiple of 128 (the K-step of the e4m3 MFMA), got {ffn_dim}")

    @staticmethod
    def _pop_reference_knobs(model_kwargs: dict, keep=()) -> None:
        for k in _IGNORED:
            if k in keep:
                continue
            v = model_kwargs.pop(k, None)
            if k in ("norm_temb",) and v:  # ... except those that change the arithmetic
                raise NotImplementedError(f"{k}={v!r} is not implemented")
            if k == "encoder_depth" and v is not None:
                raise NotImplementedError("encoder_depth is not implemented")

    def _build_engine(self, *, num_attention_heads, attention_head_dim, in_channels, out_channels, text_dim, freq_dim, ffn_dim, num_layers, eps,
                      rope_max_seq_len, chunk_size, total_num_frames, compute_dtype, enable_logvar_linear, ext=None, init_value=None, i2v=None,
                      ti2v=None, vace=None) -> None:
        """The handle (`ext`: an `fg_wan_ext_config` for fg_wan_create_ex, None: fg_wan_create; `i2v`: an `fg_wan_i2v_config` for
        fg_wan_create_i2v, `ti2v`: an `fg_wan_ti2v_config` for fg_wan_create_ti2v, `vace`: an `fg_wan_vace_config` for fg_wan_create_vace,
        each with `ext` or without) and the parameters under their state-dict paths, initial values drawn in plan order from one seeded
        generator (`init_value(name, shape, g)`, default `_init_value`)."""
        self.compute_dtype = compute_dtype
        cfg = _lib.fg_wan_config()
        cfg.compute_dtype = _lib.DTYPE_NAMES[compute_dtype or "bf16"]
        cfg.num_heads, cfg.head_dim, cfg.in_channels, cfg.out_channels = num_attention_heads, attention_head_dim, in_channels, out_channels
        cfg.text_dim, cfg.freq_dim, cfg.ffn_dim, cfg.num_layers = text_dim, freq_dim, ffn_dim, num_layers
        cfg.rope_max_seq_len, cfg.chunk_size, cfg.total_num_frames, cfg.eps = rope_max_seq_len, chunk_size, total_num_frames, eps
        self._cfg, self.in_channels = cfg, in_channels
        self._eng = _engine.Handles("wan", cfg)  # one handle: the mode is fixed at construction
        create = None
        if ext is not None or i2v is not None or ti2v is not None or vace is not None:
            def create(dt):
                c = type(cfg).from_buffer_copy(cfg)
                c.compute_dtype = dt
                h = ctypes.c_void_p()
                e = ctypes.byref(ext) if ext is not None else None
                if vace is not None:
                    _lib.check(_lib.lib().fg_wan_create_vace(ctypes.byref(c), e, ctypes.byref(vace), ctypes.byref(h)))
                elif ti2v is not None:
                    _lib.check(_lib.lib().fg_wan_create_ti2v(ctypes.byref(c), e, ctypes.byref(ti2v), ctypes.byref(h)))
                elif i2v is not None:
                    _lib.check(_lib.lib().fg_wan_create_i2v(ctypes.byref(c), e, ctypes.byref(i2v), ctypes.byref(h)))
                else:
                    _lib.check(_lib.lib().fg_wan_create_ex(ctypes.byref(c), e, ctypes.byref(h)))
                return h
        self._h = self._eng.get(cfg.compute_dtype, create)
        self._slots = {name: ConditionSlot() for name in self._SLOTS}
        g = torch.Generator().manual_seed(0)
        init = init_value or self._init_value

        def register(node, leaf, full, shp):
            if "logvar_linear" in full and not enable_logvar_linear:
                return False
            node.register_parameter(leaf, nn.Parameter(init(full, shp, g)))

        self._names, _ = _engine.build_tree(self, "wan", self._h, register)

    @staticmethod
    def _init_value(name: str, shape, g) -> torch.Tensor:
        """torch defaults of the modules diffusers builds (Linear / Conv3d: uniform(+-1/sqrt(fan_in)); RMSNorm / LayerNorm weights 1,
        biases of norms 0; scale_shift_table randn / sqrt(dim))."""
        if name.endswith("scale_shift_table"):
            return torch.randn(shape, generator=g) / shape[-1] ** 0.5
        if name.endswith(("norm_q.weight", "norm_k.weight", "norm_added_k.weight", "norm1.weight", "norm2.weight")):
            return torch.ones(shape)
        if name.endswith(("norm1.bias", "norm2.bias")):
            return torch.zeros(shape)
        fan_in = 1
        for s_ in (shape[1:] if len(shape) > 1 else shape):
            fan_in *= s_
        return (torch.rand(shape, generator=g) * 2 - 1) * fan_in ** -0.5

    # ---- library plumbing -------------------------------------------------------------------------------------------------
    _stream = staticmethod(stream)

    @property
    def _text_slot(self) -> ConditionSlot:
        return self._slots["text"]

    def _forget_text(self) -> None:
        for slot in self._slots.values():
            slot.forget()

    def _bind(self, dev: torch.device):
        names = [n for n in self._names if "logvar_linear" not in n]
        if self._eng.sync_copies(self, self._cfg.compute_dtype, names, lambda: dict(self.named_parameters()), dev):
            self._forget_text()  # the conditions on the handle were computed with the previous weights

    def fully_shard(self, **kwargs):
        """FSDP2 with the reference's grouping (Wan/network.py:761-782): one parameter group per transformer block, then the transformer
        itself (embedders - the `r_embedder` among them -, output layer, `logvar_linear`) as the root group.  The engine keeps its own
        packed bf16 copy of the weights (fastgen_amd/networks/_weights.py): a group whose parameters changed is all-gathered, packed and
        resharded - ONE block's fp32 parameters whole at a time, which is what carries to the 14B network (40 blocks of 350M parameters)."""
        from torch.distributed.fsdp import fully_shard

        tr = self._modules["transformer"]
        for block in tr._modules["blocks"]._modules.values():
            fully_shard(block, **kwargs)
        fully_shard(tr, **kwargs)

    def _ws(self, need: int, dev) -> torch.Tensor:
        return self._eng.workspace(self._cfg.compute_dtype, need, dev)

    # ---- what every call starts with ------------------------------------------------------------------------------------------
    def _no_autograd(self, *tensors) -> None:
        if torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(f"fastgen_amd.{self._NAME}: the backward pass is not implemented; call under torch.no_grad() / "
                                      "torch.inference_mode() (sampling)")

    @staticmethod
    def _text(condition: Any, what: str = "condition", who: str = "Wan") -> torch.Tensor:
        if condition is None:
            raise ValueError(f"{who} needs the text {what} [B, L, text_dim]")
        if isinstance(condition, dict):
            raise NotImplementedError("image conditioning (a condition dict) is not implemented: pass the text embeddings")
        return torch.stack(condition, dim=0) if isinstance(condition, list) else condition

    @property
    def _video_channels(self) -> int:
        return self.in_channels

    def _check_video(self, x: torch.Tensor, what: str):
        C = self._video_channels
        if x.ndim != 5 or x.shape[1] != C:
            raise ValueError(f"{what} must be [B, {C}, F, H, W], got {tuple(x.shape)}")
        return x.shape[0], x.shape[2], x.shape[3], x.shape[4]

    def _setup(self, x: torch.Tensor, what: str, workspace_bytes, *tail, key=None, bad: str = "bad video shape: {}"):
        """The video `x` (`what` in the messages) is on the GPU and shaped [B, C, F, H, W]; the weights are bound; the workspace `key`
        (default: the calls' common one) holds what `workspace_bytes(handle, B, F, H, W, *tail)` asks for - 0: the ValueError `bad`, with
        the shape in the place of {}.  Returns B, F, H, W, dev, ws."""
        _engine.require_gpu(x)
        B, F, H, W = self._check_video(x, what)
        dev = x.device
        self._bind(dev)
        need = workspace_bytes(self._h, B, F, H, W, *tail)
        if need == 0:
            raise ValueError(bad.format(f"batch {B}, frames {F}, {H}x{W} (height and width must be even)"))
        return B, F, H, W, dev, self._eng.workspace(self._cfg.compute_dtype if key is None else key, need, dev)

    @staticmethod
    def _frame_rows(v: torch.Tensor, B: int, F: int) -> torch.Tensor:
        """Timesteps in the embedder's units, [B] (or [B, F]: per frame already, the causal path), as one fp32 embedder row per frame
        (`_compute_timestep_inputs`, Wan/network.py:904-917, network_causal.py:1063-1075)."""
        v = v.to(torch.float32)
        return (v.view(-1, 1).expand(B, F) if v.ndim == 1 else v).contiguous()

    def _set_text(self, condition: torch.Tensor, B: int, dev, ws: torch.Tensor) -> None:
        """The text condition: embedded (and its cross-attention k / v cached) once per tensor, as the reference's static cache
        (the same tensor OBJECT at the same in-place version; a new object with recycled storage is embedded again)."""
        slot = self._text_slot
        if slot.same(condition):
            return
        c32 = condition.detach().to(device=dev, dtype=torch.float32).contiguous()
        if c32.shape[0] != B:
            raise ValueError(f"condition batch {c32.shape[0]} != {B}")
        _lib.check(_lib.lib().fg_wan_set_text(self._h, ptr(c32), B, c32.shape[1], ptr(ws), ws.numel(), self._stream(dev)))
        slot.remember(condition)

    # ---- the fused loops' settings ----------------------------------------------------------------------------------------------
    def _sampler_config(self, context_noise: float = 0.0, prefill_frames: int = 0):
        """The `fg_wan_sampler_config` of the student loops from the network's schedule and prediction type."""
        sc = _lib.fg_wan_sampler_config()
        rf = self.schedule_type != "edm"
        sc.t_scale = float(self.noise_scheduler.num_steps) if rf else 1.0
        sc.context_noise = float(context_noise or 0.0)
        sc.net_pred_flow = int(self.net_pred_type == "flow")
        sc.schedule = _lib.FG_SCHEDULE_RF if rf else _lib.FG_SCHEDULE_EDM
        sc.prefill_frames = int(prefill_frames)
        return sc

    def _guided_plan(self, condition: Any, neg_condition: Any, guidance_scale: Optional[float], steps: int, shift: float, solver: str, dev,
                     clamp: bool, context_noise: float = 0.0):
        """What the guided teacher samplers (`sample`) hand to their one library call: the text - [condition; neg_condition] when
        guided, that is when both guidance_scale and neg_condition are given -, `guided`, the timesteps the network sees
        (t_i = floor(1000 sigma_i) / 1000, clamped to the schedule's [min_t, max_t] under `clamp`), the filled
        `fg_wan_guided_sampler_config`, and those timesteps and the solver's table as ctypes arrays."""
        from fastgen_amd.networks.Wan import solvers

        text = condition = self._text(condition, who=self._NAME)
        guided = guidance_scale is not None and neg_condition is not None
        if guided:
            neg_condition = self._text(neg_condition, "neg_condition", self._NAME)
            if neg_condition.shape != condition.shape:
                raise ValueError(f"neg_condition {tuple(neg_condition.shape)} must be shaped like condition {tuple(condition.shape)}")
            text = torch.cat([condition.to(dev), neg_condition.to(dev)], dim=0)
        sch = self.noise_scheduler
        sigmas = solvers.flow_shift_sigmas(steps, float(shift))
        table = solvers.multistep_table(sigmas, solver, float(guidance_scale) if guided else 1.0)
        t_net = torch.floor(sigmas[:-1] * 1000.0) / 1000.0
        if clamp:
            t_net = sch.safe_clamp(t_net, min=sch.min_t, max=sch.max_t)
        sc = _lib.fg_wan_guided_sampler_config()
        sc.t_scale, sc.context_noise, sc.guidance = float(sch.num_steps), float(context_noise), int(guided)
        return (text, guided, t_net, sc, (ctypes.c_double * steps)(*t_net.tolist()),
                (ctypes.c_double * (8 * steps))(*table.reshape(-1).tolist()))
