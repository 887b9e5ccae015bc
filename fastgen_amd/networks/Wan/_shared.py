"""What the two Wan modules (`CausalWan`, network_causal.py; `Wan`, network.py) do alike with their `fg_wan_*` handle: the reference
knobs they take and refuse, the handle and the parameter tree from the library's plan, the initial values, binding, the text condition,
the workspace and `fully_shard`.  What a network does differently - its calls, its caches, its refusals - stays in its own module."""
from __future__ import annotations

import ctypes
import weakref
from typing import Optional

import torch
import torch.nn as nn

from fastgen_amd import _lib
from fastgen_amd.networks import _engine
from fastgen_amd.networks._engine import ptr, stream
from fastgen_amd.networks.network import FastGenNetwork

# reference knobs without meaning here (hub ids, autograd plumbing); a module keeps those it consumes itself (`keep`)
_IGNORED = ("model_id_or_local_path", "load_pretrained", "disable_efficient_attn", "disable_grad_ckpt", "use_fsdp_checkpoint",
            "r_embedder_init", "time_cond_type", "norm_temb", "encoder_depth", "delete_cache_on_clear")


class WanEngineNetwork(FastGenNetwork):
    """The module tree and the engine plumbing over one `fg_wan` handle (the compute mode is fixed at construction)."""

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
        self._text_key = None
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

    def _forget_text(self) -> None:
        self._text_key = None

    def _bind(self, dev: torch.device):
        names = [n for n in self._names if "logvar_linear" not in n]
        if self._eng.sync_copies(self, self._cfg.compute_dtype, names, lambda: dict(self.named_parameters()), dev):
            self._forget_text()  # the text caches were computed with the previous weights

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

    def _set_text(self, condition: torch.Tensor, B: int, dev, ws: torch.Tensor) -> None:
        """The text condition: embedded (and its cross-attention k / v cached) once per tensor, as the reference's static cache
        (the same tensor OBJECT at the same in-place version; a new object with recycled storage is embedded again)."""
        ver = 0 if condition.is_inference() else condition._version
        same = self._text_key is not None and self._text_key[0]() is condition and self._text_key[1:] == (ver, tuple(condition.shape))
        if same:
            return
        c32 = condition.detach().to(device=dev, dtype=torch.float32).contiguous()
        if c32.shape[0] != B:
            raise ValueError(f"condition batch {c32.shape[0]} != {B}")
        _lib.check(_lib.lib().fg_wan_set_text(self._h, ptr(c32), B, c32.shape[1], ptr(ws), ws.numel(), self._stream(dev)))
        self._text_key = (weakref.ref(condition), ver, tuple(condition.shape))
