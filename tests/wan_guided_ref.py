"""The guided autoregressive teacher loop of `CausalWan.sample` (reference fastgen/networks/Wan/network_causal.py:1186-1295) over the
fp32 oracle: two `oracle.wan_ref.CausalWanRef` instances that share one state dict are the two cache tags ("pos" sees the condition,
"neg" the negative condition, each with its own KV caches), and the solver is `solvers.multistep_table` applied step by step in fp64.
PARITY UNPINNED like the solver table itself (fastgen_amd/networks/Wan/solvers.py): this pins the HIP loop to the restatement."""
import torch

from fastgen_amd.networks.Wan import solvers
from oracle import wan_ref as R


def two_tags(sd, cfg=R.TINY):
    return R.CausalWanRef(sd, cfg), R.CausalWanRef(sd, cfg)


def guided_sample(pos, neg, noise, text, neg_text, guidance_scale, sample_steps, shift=5.0, solver="unipc"):
    """noise [B, C, F, H, W] -> the sample (fp64).  guidance_scale None: the unguided loop on `pos` alone."""
    sig = solvers.flow_shift_sigmas(sample_steps, shift)
    table = solvers.multistep_table(sig, solver, 1.0 if guidance_scale is None else guidance_scale)
    t_net = torch.floor(sig[:-1] * 1000.0) / 1000.0
    pos.clear_caches()
    neg.clear_caches()
    x = noise.double().clone()
    B, Fr, cs = x.shape[0], x.shape[2], pos.cfg.chunk_size
    n, rem = Fr // cs, Fr % cs
    bounds = [(0, rem)] if n == 0 else [(0 if i == 0 else cs * i + rem, cs * (i + 1) + rem) for i in range(n)]
    for a, b in bounds:
        cur, x_last, m_prev = x[:, :, a:b], None, None
        for i in range(sample_steps):
            t = t_net[i].expand(B)
            v = pos.forward(cur.float(), t, text, cur_start_frame=a, store_kv=False).double()
            vu = None
            if guidance_scale is not None:
                vu = neg.forward(cur.float(), t, neg_text, cur_start_frame=a, store_kv=False).double()
            cur, x_last, m_prev = solvers.multistep_update(table[i], cur, v, x_last, m_prev, v_uncond=vu)
        x[:, :, a:b] = cur
        t0 = torch.zeros(B, dtype=torch.float64)
        pos.forward(cur.float(), t0, text, cur_start_frame=a, store_kv=True)
        if guidance_scale is not None:
            neg.forward(cur.float(), t0, neg_text, cur_start_frame=a, store_kv=True)
    pos.clear_caches()
    neg.clear_caches()
    return x
