"""The engine-handle layer under the four network wrappers (EDMPrecond, EDM2Precond, DiT, CausalWan): everything they do alike
with a `fg_{family}_*` handle of libfastgen_amd.so - the module tree from the library's parameter plan, the handles by compute mode
with their bound weights and workspaces, the compute-mode rule, and the marshalling of tensors into library calls.  What a network
does differently (its refusals, its initial values, its calls) stays in its own module."""
from __future__ import annotations

import ctypes
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from fastgen_amd import _lib
from fastgen_amd.networks import _weights


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
def ptr(a: Optional[torch.Tensor]) -> ctypes.c_void_p:
    """Device pointer of a tensor argument; None -> null."""
    return ctypes.c_void_p(a.data_ptr() if a is not None else None)


def stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(x: torch.Tensor) -> None:
    if x.device.type != "cuda":
        raise RuntimeError("fastgen_amd runs on a HIP GPU only (no CPU path); got a tensor on " + str(x.device))


def per_sample(name: str, value: torch.Tensor, B: int, device, dtype=None) -> torch.Tensor:
    """A per-sample scalar argument (t, r, their tangents) as a contiguous [B] tensor on `device`: one entry is broadcast, any other
    count but B is refused.  dtype None keeps the value's own."""
    v = torch.atleast_1d(value.detach()).to(device=device, dtype=dtype)
    if v.numel() == 1 and B > 1:
        v = v.expand(B)
    v = v.contiguous()
    if v.numel() != B:
        raise ValueError(f"{name} has {v.numel()} entries, expected {B}")
    return v


def class_labels(condition: Optional[torch.Tensor], label_dim: int, batch: int, device) -> Optional[torch.Tensor]:
    """[B, label_dim] fp32 class labels (one row is broadcast), or None: the library then takes the embedding of zero labels, as the
    reference does (EDM/network.py:919-925)."""
    if label_dim == 0 or condition is None:
        return None
    c = condition.reshape(-1, label_dim).to(device=device, dtype=torch.float32)
    if c.shape[0] == 1 and batch > 1:
        c = c.expand(batch, -1)
    if c.shape[0] != batch:
        raise ValueError(f"condition has {c.shape[0]} rows, expected {batch}")
    return c.contiguous()


def run_x0_sampler(run, eng: "Handles", dt: int, h, n32, labels, tl_arr, steps: int, sample_type: str, loop: str, eps, seed: int, out, B: int, ws,
                   use_graph, device) -> torch.Tensor:
    """One call of `fg_sampler_run` / `fg_edm2_sampler_run` (`run`: one signature, the fused few-step loop of the two U-Nets) on the
    staging tensors of handle `dt` (`Handles.staged`): noise, labels and injected eps are copied in, and without a caller's `out` the
    result is copied out of the staged output into a tensor of the caller's.  A caller's `out` is written in place: its address is
    the caller's to keep stable."""
    n32, labels, eps = eng.staged(dt, "noise", n32), eng.staged(dt, "labels", labels), eng.staged(dt, "eps", eps)
    dst = out if out is not None else eng.staged(dt, "out", like=n32)
    _lib.check(run(h, ptr(n32), ptr(labels), tl_arr, steps, _lib.SAMPLE_TYPES[sample_type], _lib.LOOP_KINDS[loop], ptr(eps),
                   ctypes.c_uint64(seed), ptr(dst), B, ptr(ws), ws.numel(), 1 if use_graph else 0, stream(device)))
    return out if out is not None else dst.clone()


# ---- compute mode ---------------------------------------------------------------------------------------------------------------
def compute_mode(explicit: Optional[str], default: str) -> str:
    """The compute mode of a call: the module's explicit `compute_dtype`, else "bf16" under bf16 autocast, else `default` (what a
    call outside autocast, or under fp32 autocast, computes in)."""
    if explicit is not None:
        return explicit
    if torch.is_autocast_enabled():
        ad = torch.get_autocast_gpu_dtype()
        if ad == torch.bfloat16:
            return "bf16"
        if ad != torch.float32:
            raise NotImplementedError(f"autocast dtype {ad} is not implemented (bf16 or fp32)")
    return default


# ---- the module tree --------------------------------------------------------------------------------------------------------------
class _Node(nn.Module):
    """Bare container: the parameter tree only has to reproduce the reference's state-dict key paths."""


def build_tree(root: nn.Module, family: str, h, register: Callable) -> Tuple[List[str], List[Tuple[nn.Module, str]]]:
    """Walk the parameter plan of handle `h` (names, shapes and order are the library's own) and grow the `_Node` paths under
    `root`.  Every entry, in plan order, goes to `register(node, leaf_name, full_name, shape)`, which registers the parameter or
    buffer on `node` - the initial values are drawn there, so the order of the calls is the order of the RNG draws - or returns
    False to leave the entry out (nodes made for it alone are taken away again).  Returns the names kept and their
    (leaf module, leaf name) pairs."""
    L = _lib.lib()
    num, info = getattr(L, f"fg_{family}_num_params"), getattr(L, f"fg_{family}_param_info")
    name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * (5 if family == "wan" else 4))()
    names, leafs = [], []
    for i in range(num(h)):
        _lib.check(info(h, i, ctypes.byref(name), ctypes.byref(ndim), shape))
        full, shp = name.value.decode(), tuple(shape[j] for j in range(ndim.value))
        node, parts, made = root, full.split("."), []
        for p in parts[:-1]:
            if p not in node._modules:
                node.add_module(p, _Node())
                made.append((node, p))
            node = node._modules[p]
        if register(node, parts[-1], full, shp) is False:
            for parent, p in reversed(made):
                del parent._modules[p]
            continue
        names.append(full)
        leafs.append((node, parts[-1]))
    return names, leafs


# ---- the handles of one module ----------------------------------------------------------------------------------------------------
class Handles:
    """The library handles of one network module, by compute mode, with what belongs to each: the signature of the weights it has
    bound, the tensors kept alive for it, the cached workspaces (by mode, or "bwd") and the staging tensors of the fused sampler
    loops.  Destroyed with the module."""

    def __init__(self, family: str, cfg):
        self.family, self.cfg = family, cfg
        self.engines: Dict[int, ctypes.c_void_p] = {}
        self.bound_sig: Dict[int, object] = {}
        self.pack_refs: Dict[int, list] = {}
        self.ws: Dict[object, torch.Tensor] = {}
        self.staging: Dict[tuple, torch.Tensor] = {}

    def _fn(self, what: str):
        return getattr(_lib.lib(), f"fg_{self.family}_{what}")

    def create(self, dt: int) -> ctypes.c_void_p:
        """A fresh handle of compute mode `dt`, not cached (the caller destroys it)."""
        cfg = type(self.cfg).from_buffer_copy(self.cfg)
        cfg.compute_dtype = dt
        h = ctypes.c_void_p()
        _lib.check(self._fn("create")(ctypes.byref(cfg), ctypes.byref(h)))
        return h

    def get(self, dt: int, create: Optional[Callable] = None) -> ctypes.c_void_p:
        """The cached handle of compute mode `dt`, made by `create(dt)` (default: `self.create`) on first use."""
        if dt not in self.engines:
            self.engines[dt] = (create or self.create)(dt)
        return self.engines[dt]

    def destroy(self) -> None:
        try:  # (a half-constructed object, or the interpreter shutting down: nothing to report to)
            destroy = self._fn("destroy")
            while self.engines:
                destroy(self.engines.popitem()[1])
        except Exception:
            pass

    __del__ = destroy

    def workspace(self, key, need: int, device) -> torch.Tensor:
        """The cached workspace `key`, replaced when it is smaller than `need` bytes or on another device."""
        ws = self.ws.get(key)
        if ws is None or ws.numel() < need or ws.device != device:
            ws = self.ws[key] = torch.empty(need, dtype=torch.uint8, device=device)
        return ws

    def staged(self, dt: int, role: str, src: Optional[torch.Tensor] = None, like: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """The persistent device tensor of handle `dt` for argument `role` ("noise", "labels", "neg", "eps", "out", "x") of a fused
        sampler call, one per shape: the library keys its cached hipGraph on the ADDRESS of every such argument, so a call replays the
        graph only if it passes the buffers the capture saw - the callers' own tensors are new ones on every call.  `src`: copied in
        on the current stream (None, or no elements -> None: the call passes null); `like`: an output, returned as it is - the caller
        copies out of it.  Stream order on the caller's stream keeps one call's copies and launches apart from the next call's."""
        t = src if src is not None else like
        if t is None or t.numel() == 0:
            return None
        key = (dt, role, tuple(t.shape), t.dtype, t.device)
        buf = self.staging.get(key)
        if buf is None:
            with torch.inference_mode(False):  # (an inference tensor could not be written by a later call under no_grad)
                buf = self.staging[key] = torch.empty(t.shape, dtype=t.dtype, device=t.device)
        if src is not None:
            buf.copy_(src)
        return buf

    def bind_in_place(self, dt: int, names: List[str], ts: List[torch.Tensor], device) -> None:
        """For the engines that borrow the parameters' device pointers (EDM, EDM2).  Is what handle `dt` bound still what the module
        holds?  `ts` are the module's tensors in plan order, read by the caller straight from the leaf modules' parameter / buffer
        dicts - no named_parameters() generator, no per-call name -> tensor dict: this runs on every call.  Storage pointer, in-place
        version counter, dtype: any optimizer step, load_state_dict, .to() or FSDP2 all-gather changes one of them, and then every
        parameter is bound again (fp32 contiguous copies of those that are not are kept alive here) and the weights are packed."""
        sig = tuple((p.data_ptr(), p._version, p.dtype) for p in ts)
        if self.bound_sig.get(dt) == sig:
            return
        h, bind, refs = self.engines[dt], self._fn("bind_param"), []
        for n, p in zip(names, ts):
            if p.device.type != "cuda":
                raise RuntimeError(f"parameter {n} is on {p.device}; fastgen_amd runs on a HIP GPU only (no CPU path)")
            q = p.detach()
            if q.dtype != torch.float32 or not q.is_contiguous():
                q = q.to(torch.float32).contiguous()
            refs.append(q)
            _lib.check(bind(h, n.encode(), ptr(q), q.numel()))
        _lib.check(self._fn("pack_weights")(h, stream(device)))
        self.pack_refs[dt] = refs
        self.bound_sig[dt] = sig

    def sync_copies(self, owner: nn.Module, dt: int, names: List[str], tensors: Callable[[], Dict[str, torch.Tensor]], device) -> bool:
        """For the engines that copy what they are given (DiT, Wan): `_weights.sync_weights` over this family's bind / pack_group.
        True if anything was packed."""
        h, bind, pack, s = self.engines[dt], self._fn("bind_param"), self._fn("pack_group"), stream(device)
        return _weights.sync_weights(
            owner, names, self.bound_sig.setdefault(dt, {}), tensors=tensors,
            bind=lambda n, q: _lib.check(bind(h, n.encode(), ptr(q), q.numel())),
            pack_group=lambda pre, exc: _lib.check(pack(h, pre.encode(), exc.encode() if exc else None, s)))
