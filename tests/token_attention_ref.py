"""fp64 reference, error bound, structured inputs and reference mutations for the token-attention tests
(tests/test_gpu_token_attention.py).  Everything here is plain torch on whatever device the tensors live on; nothing touches the library.

Logical tensors: q [B, Lq, H * hd], k / v [B, Lkv, H * hd], bf16 values (head h in columns [h hd, (h + 1) hd))."""
import math

import torch

U = 2.0 ** -9  # unit roundoff of bf16 (8 significant bits, round to nearest)


def reference(q, k, v, H, hd):
    """softmax(q k^T / sqrt(hd)) v in fp64 of the given (bf16-valued) operands.  Returns
    want [B, Lq, H hd]; A = sum_j w_j |v_j|, same shape; T [B, Lq, H] = max_j sum_d |q_d k_jd|; top [B, Lq, H] = the scaled score
    (log2 domain, as the kernels hold it) of the leading key; lead [B, Lq, H] = its distance to the runner-up in bits (inf for one key)."""
    B, Lq, Lkv = q.shape[0], q.shape[1], k.shape[1]
    qd = q.double().view(B, Lq, H, hd).transpose(1, 2)  # [B, H, Lq, hd]
    kd = k.double().view(B, Lkv, H, hd).transpose(1, 2)
    vd = v.double().view(B, Lkv, H, hd).transpose(1, 2)
    s = qd @ kd.transpose(2, 3) * (math.log2(math.e) / math.sqrt(hd))  # bits
    w = torch.softmax(s * math.log(2.0), dim=-1)
    want = (w @ vd).transpose(1, 2).reshape(B, Lq, H * hd)
    A = (w @ vd.abs()).transpose(1, 2).reshape(B, Lq, H * hd)
    T = (qd.abs() @ kd.abs().transpose(2, 3)).amax(-1).transpose(1, 2)
    top2 = s.topk(min(2, Lkv), dim=-1).values
    top = top2[..., 0].transpose(1, 2)
    lead = (top2[..., 0] - top2[..., 1]).transpose(1, 2) if Lkv > 1 else torch.full_like(top, float("inf"))
    return dict(want=want, A=A, T=T, top=top, lead=lead)


def bound(ref, hd, Lkv, v_absmax):
    """Largest |kernel - reference| a correct kernel can show, per output element.

    With w = softmax(s) in fp64 and A = sum_j w_j |v_j|:

    bf16 terms, 3 * 2^-9 * A.  (1) each p_j is rounded to bf16 before the P V product: relative 2^-9 per term, 2^-9 A in the sum.
    (2) a row sum taken over the rounded p could be off by 2^-9 relatively, another 2^-9 A; fa_kernel, fa2_kernel (pipelined step and
    ragged tile) and fa72_seq_kernel all sum the fp32 exponentials before rounding them, so this term is not used up and covers the
    second-order products of the other two.  (3) the output's rounding to bf16: 2^-9 |out| <= 2^-9 A.  Split partials stay fp32 and
    the merge is fp32 throughout: no further bf16 rounding.

    fp32 terms.  Let d be the largest relative error of a weight before its bf16 rounding, common factors of a row aside (they cancel
    between the product and the row sum).  Numerator and row sum each carry it: 2 d A.  With T = max_j sum_d |q_d k_jd| (so |s_j| <= T),
    e = 2^-24 and 1 / sqrt(hd) nats per unit of raw score:
      score accumulation: hd fp32 additions of exact bf16 x bf16 products, |error| <= hd e T           -> hd e T / sqrt(hd)
      exponent: z = fma(s, c, -c ref) with c rounded and c ref rounded once, |z| <= 2 c T             -> 4 e T / sqrt(hd)
      a change of the running reference (at most once per key tile): alpha = exp2(c (m - m')) against the two rounded products c m,
        c m', each within e c T, and its own rounding and the multiplication by it                   -> ktiles (3 e T / sqrt(hd) + 3 e)
      exp2 itself, one ulp                                                                           -> 2 e
      row sum: a 16-term tree per tile and one addition per tile, positive terms                     -> (ktiles + 6) e
      P V accumulation in fp32, one rounding per key at worst                                        -> Lkv e
      1 / sum and the product by it                                                                  -> 3 e
      merge of the splits: lse = c m + log2(sum) (three roundings of magnitudes <= c T + 8), w = exp2(lse - max), an 8-term sum,
        the division                                                                                 -> 8 e T / sqrt(hd) + 32 e
    d <= e ((hd + 3 ktiles + 12) T / sqrt(hd) + Lkv + 4 ktiles + 43), rounded up below.
    Underflow: exponentials below 2^-126 of the row's reference flush to zero; fa2_kernel's reference may sit 2^40 below the
    maximum, so a dropped weight is below 2^-86 of the leading one: Lkv 2^-86 max|v| absolutely."""
    ktiles = (Lkv + 31) // 32
    d = 2.0 ** -24 * ((hd + 3 * ktiles + 16) * ref["T"] / math.sqrt(hd) + Lkv + 6 * ktiles + 64)  # [B, Lq, H]
    d = d.repeat_interleave(hd, dim=-1)  # per output column
    return (3 * U + 2 * d) * ref["A"] + Lkv * 2.0 ** -86 * v_absmax


def headroom(got, ref):
    """max |got - want| / (2^-9 A): 3 is the bf16 part of the bound."""
    err = (got.double() - ref["want"]).abs()
    A = ref["A"]
    return float((err[A > 0] / (U * A[A > 0])).max()) if bool((A > 0).any()) else 0.0


def round_bf16(x):
    return x.float().bfloat16()


# ---- structured inputs ------------------------------------------------------------------------------------------------------------
def edge_keys(Lkv, pieces):
    """The keys a selection input must hit: key 0, the last valid key, both neighbours of every piece boundary (split boundaries, the
    cut), and all 32 rows of an even and an odd key tile (the last two tiles that are whole; the ragged tile's keys come with them)."""
    ks = {0, Lkv - 1}
    for t0, nt in pieces:
        ks.update((32 * t0 - 1, 32 * t0, 32 * nt - 1, 32 * nt))
    whole = Lkv // 32
    for t in {0, 1, max(whole - 2, 0), max(whole - 1, 0), whole}:
        ks.update(range(32 * t, 32 * t + 32))
    return sorted(j for j in ks if 0 <= j < Lkv)


def selection(B, H, hd, Lq, Lkv, pieces, seed=0):
    """Keys are random +-1 vectors; query i of (b, h) is g k[pi(i)]: the chosen key's score leads every other by more than 30 bits, so
    out[i] = v[pi(i)] bit for bit.  pi walks edge_keys() (then every other key) in order, continuing from head to head, so that every
    query row of every query tile selects a key and consecutive rows select different ones.  Head dim 72: every odd key of the edge
    list's whole tiles differs from the key before it in dims 64 .. 67 only (the half-empty fifth contraction step tells them apart).
    Returns q, k, v (bf16) and pi [B, H, Lq]."""
    g = torch.Generator().manual_seed(1000 * seed + Lkv + Lq)
    gain = 8.0 if hd == 128 else 32.0
    k = (torch.randint(0, 2, (B, Lkv, H, hd), generator=g) * 2 - 1).float()
    if hd == 72:
        k[:, 1::2, :, :64] = k[:, 0:Lkv - (Lkv & 1):2, :, :64]
        k[:, 1::2, :, 64:68] = -k[:, 0:Lkv - (Lkv & 1):2, :, 64:68]
        k[:, 1::2, :, 68:] = k[:, 0:Lkv - (Lkv & 1):2, :, 68:]
        # (pairs (2 j, 2 j + 1) are such twins; different pairs stay random against each other)
    # |v| >= 2^-6: the other keys' share, below 2^-40 Lkv max|v|, then stays under half a bf16 ulp of v[pi(i)] (a value of exactly 0
    # would come back as that share)
    v = torch.randn(B, Lkv, H, hd, generator=g)
    v = torch.where(v.abs() < 2.0 ** -6, torch.where(v < 0, -(2.0 ** -6), 2.0 ** -6), v)
    edges = edge_keys(Lkv, pieces)
    order = torch.tensor(edges + [j for j in range(Lkv) if j not in set(edges)])
    idx = (torch.arange(B * H * Lq) % Lkv).view(B, H, Lq)
    pi = order[idx]
    q = gain * torch.gather(k.permute(0, 2, 1, 3), 2, pi[..., None].expand(B, H, Lq, hd))  # [B, H, Lq, hd]
    q = q.permute(0, 2, 1, 3).reshape(B, Lq, H * hd)
    return q.bfloat16(), k.reshape(B, Lkv, H * hd).bfloat16(), v.reshape(B, Lkv, H * hd).bfloat16(), pi


def padding_leak(B, H, hd, Lq, Lkv, seed=0):
    """Every real score is far below zero: q = -4 u, k = u + noise / 4 with u a +-1 vector per head, so a phantom key of score zero
    (a padding row that was not masked, a zero row counted by the ragged-tile path) would take the whole weight."""
    g = torch.Generator().manual_seed(2000 * seed + Lkv + Lq)
    u = (torch.randint(0, 2, (B, 1, H, hd), generator=g) * 2 - 1).float()
    q = (-4.0 * u).expand(B, Lq, H, hd) * (1.0 + 0.125 * torch.randint(0, 3, (B, Lq, H, 1), generator=g))
    k = u + 0.25 * torch.randn(B, Lkv, H, hd, generator=g)
    v = torch.randn(B, Lkv, H, hd, generator=g)
    return q.reshape(B, Lq, H * hd).bfloat16(), k.reshape(B, Lkv, H * hd).bfloat16(), v.reshape(B, Lkv, H * hd).bfloat16()


def moving_maxima(order, B, H, hd, Lq, Lkv):
    """Key norms that rise, fall or spike along the sequence (tests/test_wan.py's era test): fa2_kernel's reference maximum moves again
    and again."""
    g = torch.Generator().manual_seed(3)
    q = 4.0 * torch.randn(B, Lq, H * hd, generator=g)
    k = torch.randn(B, Lkv, H * hd, generator=g)
    ramp = torch.linspace(0.25, 8.0, Lkv)
    if order == "falling":
        ramp = ramp.flip(0)
    elif order == "spikes":
        ramp = torch.where(torch.arange(Lkv) % 97 == 5, 8.0, 0.5) * (1.0 + torch.arange(Lkv) / Lkv)
    v = torch.randn(B, Lkv, H * hd, generator=g)
    return q.bfloat16(), (k * ramp[None, :, None]).bfloat16(), v.bfloat16()


# ---- reference mutations: what a subtly wrong kernel would compute ------------------------------------------------------------------
def mutate(name, q, k, v, H, hd, arg=None):
    """The fp64 output of a kernel with one defect.  drop_last: the last valid key is not counted.  zero_key: one padding row (zero
    key, zero value) is.  swap_keys: keys arg and arg + 1 (one tile) change places in K but not in V.  shift_row: query row arg gets
    the output of row arg + 1.  drop_piece: the keys of tiles [arg[0], arg[1]) - one split's partial - are missing from the merge."""
    Lkv = k.shape[1]
    if name == "drop_last":
        return reference(q, k[:, :-1], v[:, :-1], H, hd)["want"]
    if name == "zero_key":
        z = torch.zeros_like(k[:, :1])
        return reference(q, torch.cat([k, z], 1), torch.cat([v, z], 1), H, hd)["want"]
    if name == "swap_keys":
        idx = torch.arange(Lkv)
        idx[arg], idx[arg + 1] = arg + 1, arg
        return reference(q, k[:, idx], v, H, hd)["want"]
    if name == "shift_row":
        out = reference(q, k, v, H, hd)["want"].clone()
        out[:, arg] = out[:, arg + 1]
        return out
    if name == "drop_piece":
        keep = torch.ones(Lkv, dtype=torch.bool)
        keep[32 * arg[0]:32 * arg[1]] = False
        return reference(q, k[:, keep], v[:, keep], H, hd)["want"]
    raise ValueError(name)
