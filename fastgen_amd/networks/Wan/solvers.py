"""Host side of `CausalWan.sample` (the guided autoregressive teacher sampler, reference fastgen/networks/Wan/network_causal.py:1186-1295):
the flow-matching sigma grid and the per-step coefficients of the linear multistep update that `launch_guided_multistep` (misc.hip)
applies on the device.  Everything here is float64 host arithmetic; nothing touches a GPU.

One solver step, for either solver, is the three-term form

    v      = v_uncond + g * (v_cond - v_uncond)            (guided runs only)
    m      = x_cur - s * v
    x_corr = c0 * x_last + c1 * m_prev + c2 * m            (first step: x_last := x_cur, m_prev := m - there is no history)
    x_next = p0 * x_corr + p1 * m_prev + p2 * m

and a table row holds its eight scalars `[s, g, c0, c1, c2, p0, p1, p2]`.  x_corr becomes the next step's x_last and m its m_prev.

PARITY UNPINNED.  The reference steps diffusers' `UniPCMultistepScheduler` with the scheduler config Wan publishes; diffusers is not
vendored and cannot be imported where this project is tested, so nothing pins these functions to it.  They restate, from the paper
(Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models") and from memory of that
config: data prediction (`predict_x0`) on flow sigmas (alpha = 1 - sigma), B(h) = expm1(h) ("bh2"), solver order 2, order 1 on the
first and on the last step (`lower_order_final`), final sigma 0, lambda = log((1 - sigma) / sigma).  Known differences:
  * the three-term form keeps ONE earlier data prediction, so the corrector is always UniC-1 (x_last, m_prev and the model output at the
    predicted sample); diffusers' corrector follows the preceding predictor's order and at order 2 also reads the prediction before;
  * diffusers hands the network integer timesteps `int64(1000 sigma)`; `CausalWan.sample` hands it floor(1000 sigma) / 1000 (the same
    number in the network's units), unpinned likewise.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

SOLVERS = ("unipc", "euler")


def flow_shift_sigmas(num_steps: int, shift: float, num_train_timesteps: int = 1000) -> torch.Tensor:
    """The `use_flow_sigmas` grid of diffusers' `set_timesteps`: s = 1 - linspace(1, 1 / num_train_timesteps, num_steps + 1) taken in
    descending order without its last entry (the zero), sigma = shift * s / (1 + (shift - 1) * s), then the final 0 appended:
    num_steps + 1 float64 values, strictly decreasing from shift-warped (1 - 1 / num_train_timesteps) to 0."""
    if num_steps < 1:
        raise ValueError("num_steps must be positive")
    if not shift > 0:
        raise ValueError("shift must be positive")
    s = 1.0 - torch.linspace(1.0, 1.0 / num_train_timesteps, num_steps + 1, dtype=torch.float64)
    s = torch.flip(s, dims=(0,))[:-1]
    sig = shift * s / (1.0 + (shift - 1.0) * s)
    return torch.cat([sig, torch.zeros(1, dtype=torch.float64)])


def _lam(sigma: float) -> float:
    return math.log((1.0 - sigma) / sigma)


def multistep_table(sigmas: Sequence[float], solver: str = "unipc", guidance_scale: float = 1.0) -> torch.Tensor:
    """The [steps, 8] float64 table `[s, g, c0, c1, c2, p0, p1, p2]` of the module docstring for sigmas[0] > ... > sigmas[steps] = 0.

    "euler": x_next = x + (sigma_{i+1} - sigma_i) * v.  The row holds s = sigma_i - sigma_{i+1} and the predictor (0, 0, 1): `m` is
    then the Euler point itself, x - (sigma_i - sigma_{i+1}) * v, which is the same product and sum as x + (sigma_{i+1} - sigma_i) * v
    (a negation is exact), and 0 * x_corr + 0 * m_prev + 1 * m returns it unchanged.  On the last step (sigma_{i+1} = 0) that is the
    data prediction x - sigma_i * v.  The corrector is the identity x_corr = x: (1, 0, 0) on the first step, where x_last := x, and
    (0, 1, 0) afterwards, where m_prev is the previous step's Euler point, that is x itself.

    "unipc": s = sigma_i; with alpha = 1 - sigma, h = lambda_next - lambda_i, E = expm1(-h):
      predictor, order 1 (first and last step):  x_next = (sigma_next / sigma_i) x_corr - alpha_next E m
      predictor, order 2, r = (lambda_{i-1} - lambda_i) / h:  ... - alpha_next E (m + (m_prev - m) / (2 r))
      corrector (from the second step on), h' = lambda_i - lambda_{i-1}, E' = expm1(-h'):
                 x_corr = (sigma_i / sigma_{i-1}) x_last - alpha_i E' (m_prev + (m - m_prev) / 2)
    The last step lands on sigma = 0 where h is infinite: E = -1, the sigma ratio 0, so x_next = m."""
    if solver not in SOLVERS:
        raise NotImplementedError(f"solver must be one of {SOLVERS}, got {solver!r}")
    sg = [float(v) for v in (sigmas.tolist() if isinstance(sigmas, torch.Tensor) else sigmas)]
    steps = len(sg) - 1
    if steps < 1:
        raise ValueError("sigmas must hold at least two values")
    if sg[-1] != 0.0 or any(not (sg[i] > sg[i + 1]) for i in range(steps)) or not sg[0] < 1.0:
        raise ValueError("sigmas must decrease strictly from below 1 to a final 0")
    g = float(guidance_scale)
    rows = []
    for i in range(steps):
        s_i, s_n = sg[i], sg[i + 1]
        if solver == "euler":
            rows.append([s_i - s_n, g] + ([1.0, 0.0, 0.0] if i == 0 else [0.0, 1.0, 0.0]) + [0.0, 0.0, 1.0])
            continue
        c = [1.0, 0.0, 0.0]
        if i > 0:
            e = math.expm1(-(_lam(s_i) - _lam(sg[i - 1])))
            a = (1.0 - s_i) * e
            c = [s_i / sg[i - 1], -0.5 * a, -0.5 * a]
        if s_n == 0.0:
            p = [0.0, 0.0, 1.0]
        else:
            h = _lam(s_n) - _lam(s_i)
            a = (1.0 - s_n) * math.expm1(-h)
            if i == 0:  # order 1: no history (i == steps - 1 is the s_n == 0 branch)
                p = [s_n / s_i, 0.0, -a]
            else:
                r = (_lam(sg[i - 1]) - _lam(s_i)) / h
                p = [s_n / s_i, -a * 0.5 / r, -a + a * 0.5 / r]
        rows.append([s_i, g] + c + p)
    return torch.tensor(rows, dtype=torch.float64)


def multistep_update(row: torch.Tensor, x_cur: torch.Tensor, v: torch.Tensor, x_last: Optional[torch.Tensor] = None,
                     m_prev: Optional[torch.Tensor] = None, v_uncond: Optional[torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One table row applied in the tensors' own dtype, in the operation order of `launch_guided_multistep`: the scalars rounded once to
    that dtype, every product and sum an operation of its own (no fused multiply-add).  On float32 tensors this is the kernel bit for bit;
    on float64 tensors it is the reference.  x_last / m_prev None: the first step.  v_uncond given: v is the conditional flow.
    Returns (x_next, x_corr, m)."""
    s, g, c0, c1, c2, p0, p1, p2 = row.to(torch.float64).to(x_cur.dtype).tolist()
    if v_uncond is not None:
        d = v - v_uncond
        v = v_uncond + g * d
    m = x_cur - s * v
    if x_last is None:
        x_last, m_prev = x_cur, m
    x_corr = c0 * x_last
    x_corr = x_corr + c1 * m_prev
    x_corr = x_corr + c2 * m
    x_next = p0 * x_corr
    x_next = x_next + p1 * m_prev
    x_next = x_next + p2 * m
    return x_next, x_corr, m
