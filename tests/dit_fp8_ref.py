"""Torch mirror of the fp8 compute mode's quantiser (include/fastgen_amd.h, FG_DTYPE_FP8; gemm.hip quant_rows_fp8_kernel, dit.hip
ln_modulate_kernel's quantising store) and a fake-quant oracle of the DiT: oracle/dit_ref.py's block with the four block linears (qkv,
attention.proj, fc1, fc2) replaced by F.linear(dq(q(x)), dq(q(W)), b) - operands quantised row by row (W: per output channel, x: per token) and
dequantised again, the product itself in the caller's precision.  Imported from tests only.

Row scheme (W8A8, dynamic): amax = max |x| over the row; amax == 0: scale = 1, q = 0; else scale = amax / 448.0f, inv = 448.0f / amax
(two IEEE fp32 divisions; inv is NOT 1 / scale) and q = e4m3fn_RNE(clamp(x * inv, -448, 448)) - OCP e4m3fn, what torch.float8_e4m3fn is."""
import math

import torch
import torch.nn.functional as F

from oracle import dit_ref as R

# relative L2 distance of the fake-quant oracle (fp32) from the reference-recorded golden output (tests/golden/dit_forward_b2.pt);
# tests/test_fp8_ref.py pins these values, the GPU tests bound the fp8 forward by twice them
E_Q = {"s": 0.0469, "xl": 0.0538}


def quant_rows(x: torch.Tensor):
    """x [..., K] (fp32, fp64 or bf16; widened / narrowed to fp32 first) -> (q [..., K] float8_e4m3fn, scale [...] fp32)."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1, keepdim=True)
    zero = amax == 0
    c448 = torch.full_like(amax, 448.0)  # (tensor / tensor: a true fp32 division on every backend)
    safe = torch.where(zero, c448, amax)
    scale = torch.where(zero, torch.ones_like(amax), safe / c448)
    inv = torch.where(zero, torch.ones_like(amax), c448 / safe)
    q = (xf * inv).clamp(-448, 448).to(torch.float8_e4m3fn)
    return q, scale.squeeze(-1)


def dequant(q: torch.Tensor, scale: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    return q.to(dtype) * scale.to(dtype).unsqueeze(-1)


def fake_quant(x: torch.Tensor) -> torch.Tensor:
    """dq(q(x)) in x's dtype (fp32 / fp64: every e4m3 value times an fp32 scale is exact in either)."""
    q, s = quant_rows(x)
    return dequant(q, s, x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32)


class FakeQuantWeights:
    """The four block linears' weights of a state dict, fake-quantised once per tensor."""

    def __init__(self, sd):
        self.sd, self._fq = sd, {}

    def linear(self, x, wname, bname):
        if wname not in self._fq:
            self._fq[wname] = fake_quant(self.sd[wname])
        return F.linear(fake_quant(x), self._fq[wname], self.sd[bname])


def dit_block_fq(fq: FakeQuantWeights, i: int, x: torch.Tensor, c: torch.Tensor, heads: int) -> torch.Tensor:
    """oracle.dit_ref.dit_block with quantised operands in qkv / proj / fc1 / fc2 (the conditioning linear stays as it is)."""
    sd, b = fq.sd, f"blocks.{i}."
    p = F.linear(F.silu(c), sd[b + "conditioning_net.1.weight"], sd[b + "conditioning_net.1.bias"]).chunk(6, dim=1)
    a_shift, a_scale, a_gate, f_shift, f_scale, f_gate = p
    h = R.modulate(R.layer_norm(x), a_shift, a_scale)
    B, N, D = h.shape
    hd = D // heads
    qkv = fq.linear(h, b + "attention.qkv.weight", b + "attention.qkv.bias").reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    att = ((q * hd ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
    o = (att @ v).transpose(1, 2).reshape(B, N, D)
    x = x + a_gate.unsqueeze(1) * fq.linear(o, b + "attention.proj.weight", b + "attention.proj.bias")
    h = R.modulate(R.layer_norm(x), f_shift, f_scale)
    h = F.gelu(fq.linear(h, b + "feed_forward.fc1.weight", b + "feed_forward.fc1.bias"), approximate="tanh")
    h = fq.linear(h, b + "feed_forward.fc2.weight", b + "feed_forward.fc2.bias")
    return x + f_gate.unsqueeze(1) * h


def dit_forward_fq(sd, cfg, x_t: torch.Tensor, t: torch.Tensor, condition: torch.Tensor) -> torch.Tensor:
    """oracle.dit_ref.dit_forward (no r, no SiT convention) with dit_block_fq for the blocks."""
    assert not cfg.r_timestep and not cfg.use_sit_convention
    if condition.ndim == 2:
        mask = torch.any(condition != 0, dim=1)
        condition = torch.where(~mask, cfg.num_classes, condition.argmax(dim=1))
    t_ = ((t * 1000.0) if cfg.scale_t else t).to(x_t.dtype)
    x = R.patch_embed(sd, cfg, x_t)
    c = R.time_embedding(sd, "t_embedder", t_) + sd["y_embedder.class_embeddings.weight"][condition]
    fq = FakeQuantWeights(sd)
    for i in range(cfg.depth):
        x = dit_block_fq(fq, i, x, c, cfg.num_heads)
    return R.final_layer(sd, cfg, x, c)
