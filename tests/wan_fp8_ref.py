"""Fake-quant oracle of the causal video DiT's fp8 compute mode (`CausalWan(compute_dtype="fp8")`, include/fastgen_amd.h fg_wan_config):
oracle/wan_ref.py with the six block linears that read the video tokens - attn1.to_q / to_k / to_v (one fused GEMM in the engine; rows
are independent, so quantising the three weights apart is the same), attn1.to_out.0, attn2.to_q, attn2.to_out.0, ffn.net.0.proj,
ffn.net.2 - replaced by F.linear(dq(q(x)), dq(q(W)), b): operands quantised row by row (W per output channel, x per token) by the mirror
of tests/dit_fp8_ref.py and dequantised again, the product in the caller's precision.  Every other linear (text side, embedders,
proj_out) stays as it is.  Imported from tests only.

`fake_quant_oracle(mutant)` is a context manager that swaps `oracle.wan_ref._lin` for that version while it is open.  The MUTANTS are
four quantisation schemes an engine could follow by mistake; the GPU test asks the fp8 output to be closer to the stated scheme than to
each of them.

The two configurations of tests/test_gpu_wan_fp8.py, their seeded inputs and the three network calls per configuration (`CALLS`) live
here, so that the CPU test that pins E_Q and the GPU test that uses it run the same oracle on the same numbers (computed once per
process: `oracle_outputs`)."""
import contextlib
import functools

import torch
import torch.nn.functional as F

import dit_fp8_ref as Q
from oracle import wan_ref as R

FP8_LINEARS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_out.0", "ffn.net.0.proj", "ffn.net.2")
MUTANTS = ("per_tensor_act", "weights_unquantised", "no_ffn2", "amax_240")

# "reg": every GEMM on the register-staged kernel (M = 128 / 384 tokens, 64 per frame).  "pp": the smallest shape at which the ping-pong
# kernel and its two-gate-row token epilogue run (M = 512, 256 tokens per frame = one gate row per 256-row tile half).
CONFIGS = {
    "reg": dict(cfg=R.TINY, hw=16, text_len=16, seed=61),
    "pp": dict(cfg=R.WanConfig(num_heads=3, head_dim=128, text_dim=128, ffn_dim=1024, num_layers=2, chunk_size=2, total_num_frames=4),
               hw=32, text_len=16, seed=62),
}
CALLS = ("ar0", "ar1", "bc")  # chunk 0 with store_kv; chunk 1 over that cache; the block-causal call over all frames

# E_Q[tag][call]: relative L2 of the fake-quant oracle from the plain oracle, both fp64 (tests/test_wan_fp8_ref.py pins these to 5 %;
# the GPU test bounds the fp8 output's distance from the PLAIN oracle by twice them).  Random weights: the network's parity is unpinned.
E_Q = {
    "reg": {"ar0": 0.0202, "ar1": 0.0194, "bc": 0.0197},
    "pp": {"ar0": 0.0196, "ar1": 0.0213, "bc": 0.0205},
}


def _fake_quant_top(x: torch.Tensor, top: float) -> torch.Tensor:
    """The row scheme with amax mapped to `top` instead of 448 (240 is the largest value of the OTHER 8-bit e4m3 flavour, e4m3fnuz)."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1, keepdim=True)
    zero = amax == 0
    ctop = torch.full_like(amax, top)
    safe = torch.where(zero, ctop, amax)
    scale = torch.where(zero, torch.ones_like(amax), safe / ctop)
    inv = torch.where(zero, torch.ones_like(amax), ctop / safe)
    q = (xf * inv).clamp(-top, top).to(torch.float8_e4m3fn)
    return q.to(x.dtype) * scale.to(x.dtype)


def _per_tensor(x: torch.Tensor) -> torch.Tensor:
    """One scale for the whole activation tensor instead of one per token."""
    return Q.fake_quant(x.reshape(1, -1)).reshape(x.shape)


@contextlib.contextmanager
def fake_quant_oracle(mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    plain, cache = R._lin, {}
    fq_x = _per_tensor if mutant == "per_tensor_act" else (lambda x: _fake_quant_top(x, 240.0)) if mutant == "amax_240" else Q.fake_quant
    fq_w = (lambda w: w) if mutant == "weights_unquantised" else (lambda w: _fake_quant_top(w, 240.0)) if mutant == "amax_240" else Q.fake_quant

    def lin(p, x, name):
        if not name.startswith("blocks.") or not name.endswith(FP8_LINEARS) or (mutant == "no_ffn2" and name.endswith("ffn.net.2")):
            return plain(p, x, name)
        key = (id(p), name)
        if key not in cache:
            cache[key] = fq_w(p[name + ".weight"])
        return F.linear(fq_x(x), cache[key], p[name + ".bias"])

    R._lin = lin
    try:
        yield
    finally:
        R._lin = plain


@functools.lru_cache(maxsize=None)
def case(tag):
    """(cfg, state dict, x [1, 16, F, hw, hw], text [1, Lt, text_dim], t of the three calls) of a configuration, seeded."""
    c = CONFIGS[tag]
    cfg = c["cfg"]
    g = torch.Generator().manual_seed(c["seed"])
    sd = R.random_state_dict(cfg, c["seed"])
    x = torch.randn(1, cfg.in_channels, cfg.total_num_frames, c["hw"], c["hw"], generator=g)
    text = torch.randn(1, c["text_len"], cfg.text_dim, generator=g)
    t_bc = torch.rand(1, cfg.total_num_frames, generator=g, dtype=torch.float64) * 0.9 + 0.05  # one timestep per frame: diffusion forcing
    ts = {"ar0": torch.tensor([0.3], dtype=torch.float64), "ar1": torch.tensor([0.6], dtype=torch.float64), "bc": t_bc}
    return cfg, sd, x, text, ts


def run_calls(tag, forward):
    """The three calls of CALLS through `forward(x, t, text, cur_start_frame, store_kv, block_causal)`, in order (ar1 reads ar0's cache)."""
    cfg, _, x, text, ts = case(tag)
    cs = cfg.chunk_size
    return {"ar0": forward(x[:, :, :cs], ts["ar0"], text, 0, True, False),
            "ar1": forward(x[:, :, cs:2 * cs], ts["ar1"], text, cs, False, False),
            "bc": forward(x, ts["bc"], text, 0, False, True)}


@functools.lru_cache(maxsize=None)
def oracle_outputs(tag, mode):
    """fp64 outputs {call: [1, C, F, H, W]} of the plain oracle (mode "plain"), the fake-quant oracle ("fq") or a mutant of it."""
    cfg, sd, _, _, _ = case(tag)
    net = R.CausalWanRef(sd, cfg, dtype=torch.float64)
    ctx = contextlib.nullcontext() if mode == "plain" else fake_quant_oracle(None if mode == "fq" else mode)
    with torch.no_grad(), ctx:
        return run_calls(tag, lambda x, t, text, start, store, bc: net.forward(x, t, text, cur_start_frame=start, store_kv=store, block_causal=bc))


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).norm() / b.double().norm())
