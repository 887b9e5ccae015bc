"""fp64 reference, per-element bounds, structured inputs, operand packing and reference mutations for the DiT attention kernels
(fastgen_amd/csrc/dit.hip: dit_attention_kernel, the whole-sequence form at 256 tokens, and dit_flash_kernel, the online softmax over
blocks of KB = 128 keys) - tests/test_dit_attention_ref.py on the CPU, tests/test_gpu_dit_flash_attention.py through fg_op_dit_attention.

Logical tensors as in tests/token_attention_ref.py: q, k, v [B, T, H * hd] (head h in columns [h hd, (h + 1) hd)).  The reference and the
bf16 bound are that file's (`reference`, `bound`).

Split-bf16 flavour (FG_DTYPE_BF16X3).  An operand x is the pair hi = bf16(x), lo = bf16(x - hi) and a product a b is evaluated as
a_lo b_hi + a_hi b_lo + a_hi b_hi with fp32 accumulation.  With 8 significant bits, |x - hi| <= 2^-8 |x|, so |lo| <= 2^-8 |x| (to first
order) and |x - hi - lo| <= 2^-16 |x|.  The tests hand the kernel q, k, v as planes and take the reference of hi + lo, so q, k and v carry
no rounding of their own; P is split inside the kernel.  In the notation of token_attention_ref.bound (w = softmax in fp64,
A = sum_j w_j |v_j|, T = max_j sum_d |q_d k_jd|, e = 2^-24, d = the largest relative error of a weight, which numerator and row sum each
carry: 2 d A):
  scores     the dropped q_lo k_lo products: |q_lo k_lo| <= 2^-16 |q k| per term, 2^-16 T per score     -> d += 2^-16 T / sqrt(hd)
             three fp32-accumulated products per dim instead of one                                       -> hd e T becomes 3 hd e T
  P V        P = [hi | lo] to 2^-16 relatively, and the dropped p_lo v_lo products, 2^-16 per term        -> 2 * 2^-16 A
             three accumulated products per key                                                           -> Lkv e becomes 3 Lkv e
  output     stored as fp32: one rounding, e |out| <= e A, inside the constant of d
  the other fp32 terms (exponent, change of the running reference once per key block, exp2, row sum, 1 / sum) as listed there, with
  ktiles = the number of key blocks.
So d3 = e ((3 hd + 3 kblocks + 16) T / sqrt(hd) + 3 Lkv + 6 kblocks + 64) + 2^-16 T / sqrt(hd) and
bound = (2^-15 + 2 d3) A + Lkv 2^-86 max|v|.  There is no bf16 term: nothing in this flavour is rounded to 8 bits."""
import math

import torch

from token_attention_ref import bound as _bound_tiles32
from token_attention_ref import reference, selection  # noqa: F401  (re-exported)

KB = 128  # keys per block of dit_flash_kernel
E = 2.0 ** -24


def kblocks(T, path_flash):
    """Changes of the running reference a kernel can make: one per key block; the whole-sequence kernel has a single maximum."""
    return T // KB if path_flash else 1


def bound_bf16(ref, hd, T, v_absmax, nblocks):
    """token_attention_ref.bound with ktiles = nblocks.  That function counts one change of reference per 32 keys (its kernels' tile); the
    terms in ktiles are linear, so the difference is taken off again: d -= e (3 T / sqrt(hd) + 6) (ceil(Lkv / 32) - nblocks)."""
    extra = (T + 31) // 32 - nblocks
    dd = E * (3 * extra * ref["T"] / math.sqrt(hd) + 6 * extra)
    return _bound_tiles32(ref, hd, T, v_absmax) - 2 * dd.repeat_interleave(hd, dim=-1) * ref["A"]


def bound_x3(ref, hd, T, v_absmax, nblocks):
    d = E * ((3 * hd + 3 * nblocks + 16) * ref["T"] / math.sqrt(hd) + 3 * T + 6 * nblocks + 64) + 2.0 ** -16 * ref["T"] / math.sqrt(hd)
    d = d.repeat_interleave(hd, dim=-1)
    return (2.0 ** -15 + 2 * d) * ref["A"] + T * 2.0 ** -86 * v_absmax


def bound(mode, ref, hd, T, v_absmax, nblocks):
    return (bound_x3 if mode == "bf16x3" else bound_bf16)(ref, hd, T, v_absmax, nblocks)


# ---- operand values as a mode sees them ---------------------------------------------------------------------------------------------
def split(x):
    """hi, lo bf16 planes of an fp32 tensor (common.h split8: round to nearest even both times)."""
    hi = x.float().bfloat16()
    lo = (x.float() - hi.float()).bfloat16()
    return hi, lo


def as_seen(mode, x):
    """The fp64 value of an operand as the kernel of `mode` reads it: bf16(x), or hi + lo."""
    if mode == "bf16":
        return x.float().bfloat16().double()
    hi, lo = split(x)
    return hi.double() + lo.double()


def heads_first(x, H, hd):
    B, T = x.shape[:2]
    return x.view(B, T, H, hd).permute(0, 2, 1, 3).contiguous()  # [B, H, T, hd]


def pack(mode, q, k, v, H, hd):
    """The op's operand buffers: q, k [B][H][T][hd]; vt [B][H][hd][T] followed by 32 * T elements of slack; in the split mode each a hi
    plane and a lo plane lo_off = B H T hd + 32 T elements apart.  Returns (q, k, vt) bf16 tensors (1-D) and lo_off (0 in the bf16 mode)."""
    B, T = q.shape[:2]
    n = B * H * T * hd
    lo_off = n + 32 * T
    planes = []
    for x in (heads_first(q, H, hd), heads_first(k, H, hd), heads_first(v, H, hd).transpose(2, 3).contiguous()):
        if mode == "bf16":
            buf = torch.zeros(lo_off, dtype=torch.bfloat16)
            buf[:n] = x.float().bfloat16().reshape(-1)
        else:
            hi, lo = split(x)
            buf = torch.zeros(2 * lo_off, dtype=torch.bfloat16)
            buf[:n] = hi.reshape(-1)
            buf[lo_off:lo_off + n] = lo.reshape(-1)
        planes.append(buf)
    return planes[0], planes[1], planes[2], (0 if mode == "bf16" else lo_off)


# ---- structured inputs (fp32 values; a mode sees them through as_seen) ----------------------------------------------------------------
def gaussian(B, H, hd, T, seed=0):
    g = torch.Generator().manual_seed(4000 + 10 * T + hd + seed)
    return tuple(torch.randn(B, T, H * hd, generator=g) for _ in range(3))


def spiked(where, B, H, hd, T, seed=0, gain=3.0):
    """Gaussian q / k / v; for the chosen queries (one per 32-query slab of every head, walking the slab's rows) one key row of the
    last ("late") or first ("early") key block is gain * q: that key leads the query's row by many bits.  Returns q, k, v and the
    (b, h, query, key) quadruples."""
    q, k, v = gaussian(B, H, hd, T, seed + 1)
    k4, q4 = k.view(B, T, H, hd), q.view(B, T, H, hd)
    picks = []
    for b in range(B):
        for h in range(H):
            for slab in range(T // 32):
                qi = 32 * slab + (5 * slab + 3 * h + b) % 32
                kj = (T - KB if where == "late" else 0) + (37 * slab + 11 * h + 64 * b) % KB  # (37 is odd: distinct keys for the <= 32 slabs)
                picks.append((b, h, qi, kj))
    assert len({(b, h, kj) for b, h, _, kj in picks}) == len(picks)
    for b, h, qi, kj in picks:
        k4[b, kj, h] = gain * q4[b, qi, h]
    return q, k, v, picks


def all_equal(B, H, hd, T, seed=0):
    """Every key of a head is the same row: uniform weights, the output is the mean of v."""
    q, k, v = gaussian(B, H, hd, T, seed + 2)
    k = k[:, :1].expand(B, T, H * hd).contiguous()
    return q, k, v


def block_selection(B, H, hd, T, seed=0):
    """token_attention_ref.selection with the key blocks as pieces: key 0, key T - 1 and both neighbours of every block boundary."""
    pieces = [(4 * i, 4 * i + 4) for i in range(T // KB)]
    q, k, v, pi = selection(B, H, hd, T, T, pieces, seed=seed)
    return q.float(), k.float(), v.float(), pi


def two_level(B, H, hd, T):
    """One key per head scores 1 nat (hd 64; 1.06 at 72) above all the others, which score 0, and v > 0: every weight but the leading
    one is exp(-1) = 0.3679, 0.35 ulp away from its bf16 neighbour - rounding P to bf16 shifts the output by 1.9e-3 relatively, all in
    one direction.  Exact in bf16, T = sum |q k| = hd / 8: the score terms of the bounds are small."""
    g = torch.Generator().manual_seed(77 + T + hd)
    u = (torch.randint(0, 2, (B, 1, H, hd), generator=g) * 2 - 1).float()
    q = u.expand(B, T, H, hd).reshape(B, T, H * hd).contiguous()
    k = torch.zeros(B, T, H, hd)
    k[:, 5] = u[:, 0] / 8
    v = (torch.rand(B, T, H * hd, generator=g) + 0.5).bfloat16().float()
    return q, k.reshape(B, T, H * hd), v


# ---- the flash form in fp64, with optional defects -------------------------------------------------------------------------------------
def flash_fp64(q, k, v, H, hd, defect=None, kb=KB):
    """Online softmax over key blocks of kb in fp64 on [B, T, H hd] tensors: what dit_flash_kernel computes, rounding aside.  defect:
      "no_rescale"    O and the row sum stay at the old maximum when the maximum moves
      "rescale_l"     the row sum is rescaled, O is not
      "p_bf16"        P is rounded to bf16 before P V (the row sum is of the unrounded weights, as in the kernels)
      "p_split"       P is rounded to hi + lo (what the split mode does: NOT a defect)"""
    B, T = q.shape[:2]
    qd = q.double().view(B, T, H, hd).transpose(1, 2)
    kd = k.double().view(B, T, H, hd).transpose(1, 2)
    vd = v.double().view(B, T, H, hd).transpose(1, 2)
    m = torch.full((B, H, T, 1), -math.inf, dtype=torch.float64)
    l = torch.zeros(B, H, T, 1, dtype=torch.float64)
    o = torch.zeros(B, H, T, hd, dtype=torch.float64)
    for j in range(0, T, kb):
        s = qd @ kd[:, :, j:j + kb].transpose(2, 3) / math.sqrt(hd)
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)
        p = torch.exp(s - mn)
        l = (l if defect == "no_rescale" else l * alpha) + p.sum(-1, keepdim=True)
        if defect == "p_bf16":
            p = p.float().bfloat16().double()
        elif defect == "p_split":
            hi, lo = split(p)
            p = hi.double() + lo.double()
        o = (o if defect in ("no_rescale", "rescale_l") else o * alpha) + p @ vd[:, :, j:j + kb]
        m = mn
    return (o / l).transpose(1, 2).reshape(B, T, H * hd)
