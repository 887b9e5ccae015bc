"""`FastGenNetwork` duck type: the nn.Module surface the reference's methods / trainer / inference scripts
call (fastgen/networks/network.py:13-208).  The 'edm' and 'rf' schedules exist on this path."""
from __future__ import annotations

import ctypes
from abc import ABC, abstractmethod
from typing import Any, Optional

import torch

from fastgen_amd import _lib
from fastgen_amd.networks.noise_schedule import NET_PRED_TYPES, expand_like, get_noise_schedule


class FastGenNetwork(ABC, torch.nn.Module):
    def __init__(self, net_pred_type: str = "x0", schedule_type: str = "edm", **net_kwargs):
        super().__init__()
        if net_pred_type not in NET_PRED_TYPES:
            raise ValueError(f"Unsupported net_pred_type '{net_pred_type}'. Supported types are: {NET_PRED_TYPES}")
        self.net_pred_type = net_pred_type
        self.schedule_type = schedule_type
        self.set_noise_schedule(**net_kwargs)

    def set_noise_schedule(self, schedule_type: Optional[str] = None, **kw) -> None:
        if schedule_type is not None:
            self.schedule_type = schedule_type
        self.noise_scheduler = get_noise_schedule(self.schedule_type, **kw)

    def reset_parameters(self):
        if getattr(self, "noise_scheduler", None) is not None:
            self.set_noise_schedule()

    def fully_shard(self, **kwargs):
        raise NotImplementedError(f"Network {self.__class__.__name__} does not implement the fully_shard method.")

    def sample(self, noise: torch.Tensor, condition: Optional[Any] = None, neg_condition: Optional[Any] = None,
               guidance_scale: Optional[float] = 5.0, num_steps: int = 50, **kwargs) -> torch.Tensor:
        raise NotImplementedError(f"Network {self.__class__.__name__} does not implement the sample method.")

    @abstractmethod
    def forward(self, x_t, t, condition=None, r=None, return_features_early=False, feature_indices=None,
                return_logvar=False, fwd_pred_type=None, **fwd_kwargs):
        ...


def _fused_sample_args(noise: torch.Tensor, t_list, sample_type: str, eps: Optional[torch.Tensor], seed: Optional[int],
                       n_eps: Optional[int] = None):
    """The checks and conversions every `few_step_sample` makes before its library call: noise on the GPU, a known sample_type,
    t_list ending in 0, `eps` holding steps-1 (or `n_eps`) noise tensors shaped like `noise`, a seed drawn from the host RNG (it follows
    torch.manual_seed / set_random_seed) when none is given.  Returns (fp32 contiguous noise, steps, t_list as a ctypes double array,
    eps as fp32 contiguous on noise's device or None, seed)."""
    if noise.device.type != "cuda":
        raise RuntimeError("fastgen_amd runs on a HIP GPU only (no CPU path); got a tensor on " + str(noise.device))
    if sample_type not in _lib.SAMPLE_TYPES:
        raise NotImplementedError(f"student_sample_type must be one of 'sde', 'ode' but got {sample_type}")
    tl = [float(v) for v in (t_list.tolist() if isinstance(t_list, torch.Tensor) else t_list)]
    steps = len(tl) - 1
    assert tl[-1] == 0, "t_list[-1] must be zero"
    n32 = noise if (noise.dtype == torch.float32 and noise.is_contiguous()) else noise.to(torch.float32).contiguous()
    if eps is not None:
        eps = eps.to(device=noise.device, dtype=torch.float32).contiguous()
        if eps.numel() != (max(steps - 1, 0) if n_eps is None else n_eps) * n32.numel():
            raise ValueError(f"eps must hold steps-1 = {steps - 1} noise tensors shaped like `noise`")
    if seed is None:
        seed = int(torch.randint(0, 2**62, (1,)).item())
    return n32, steps, (ctypes.c_double * (steps + 1))(*tl), eps, seed


def _edm_euler_sample(net: FastGenNetwork, noise: torch.Tensor, condition, neg_condition, guidance_scale: Optional[float],
                      num_steps: int) -> torch.Tensor:
    """Deterministic Euler sampler of an EDM-schedule teacher with optional classifier-free guidance (EDM/network.py:976-1026), one
    forward() per step: `sample()` of EDMPrecond and EDM2Precond."""
    assert net.schedule_type == "edm", f"{net.schedule_type} is not supported"
    sigmas = net.noise_scheduler.get_t_list(num_steps, device=noise.device)
    x = net.noise_scheduler.latents(noise=noise, t_init=sigmas[0])
    for sigma, sigma_next in zip(sigmas[:-1], sigmas[1:]):
        t = sigma.expand(x.shape[0])
        if guidance_scale is not None and guidance_scale > 1.0 and neg_condition is not None:
            x0 = net(torch.cat([x, x], 0), torch.cat([t, t], 0), condition=torch.cat([neg_condition, condition], 0), fwd_pred_type="x0")
            x0_uncond, x0_cond = x0.chunk(2)
            x0 = x0_uncond + guidance_scale * (x0_cond - x0_uncond)
        else:
            x0 = net(x, t, condition=condition, fwd_pred_type="x0")
        d = (x - x0) / expand_like(t, x)
        x = x + (sigma_next - sigma).to(x.dtype) * d
    return x
