"""Plain fp64 references of the SongUNet (EDMPrecond) INFERENCE kernels - conv.hip, conv_ws.hip, conv_ws3.hip, the GroupNorm finalize /
pool / stem / head kernels of misc.hip and aux.hip, attn.hip - restated from those files' header comments and the reference network's
arithmetic (EDM/network.py), never from the kernels' index code.  Each returns (value, bound): `bound` is a per-element bound of what the
kernel's own arithmetic may differ from `value` by; the tests assert |got - ref| <= bound for EVERY element.

`mode` is the compute mode: 0 fp32 (exact fp32 products), 1 bf16 (bf16 tensors, operands and weights; fp32 accumulation), 2 bf16x3 (fp32
tensors, every product hi*hi + hi*lo + lo*hi of bf16 halves).  The reference rounds where the headers say the kernel rounds - the bf16
operand and weights of mode 1, the bf16 store - so a comparison isolates indexing and accumulation from the declared roundings.

How a bound is built (the conventions of tests/edm_train_ref.py, whose primitives are used).  A sum of n terms, in any order, contributes
u (n + 2) sum|terms|, u = 2^-24.  A split-bf16 product drops a_lo b_lo and the two third-level residues, each <= 2^-18 |a b| (common.h):
X3 = 3 * 2^-18 per product, and its three partial products make the sum 3 n terms long.  The sigmoid term is edm_train_ref._sigmoid_err.
A bf16 store contributes the exact half ulp of the value; an operand the kernel rounds to bf16 AFTER computing it in fp32 is rounded by
the reference too and charged one flip (edm_train_ref.stored) where its value lies within the carried error of a rounding tie.  Every
stage's error is carried to first order through the later ones (|d f / d x| dx in absolute value); the one place first order is not
enough - 1 / sqrt(var + eps) at a large mean offset - uses the exact worst case.

The conv is torch.nn.functional.conv2d in fp64 on the explicitly built operand: concat [src1 | src2] -> a x + b (-> SiLU) per `pro` ->
resample (nearest 2x for RES_UP / RES_SUBPIX, the 2x2 mean for RES_DOWN) -> zero padding; then + bias + temb[n] + resid (rshift: the
half-resolution pixel (y >> 1, x >> 1)), * scale.  `mut` names a mutation of a reference: what a subtly wrong kernel would compute
(MUTANTS); tests/test_edm_ops_ref.py shows on the CPU that each lies at least 5 bounds away on a named case."""
import math

import torch
import torch.nn.functional as F

from edm_train_ref import F64, U, _sigmoid_err, bf16_round, final, gn_geometry, stored

X3 = 3.0 * 2.0 ** -18
E64 = 2.0 ** -50          # what the fp64 stages of a kernel (slot combination, weight merge) may lose, relative to sum|terms|
TINY = 2.0 ** -120        # results below fp32's normal range are flushed by v_exp / v_rcp
PRO_NONE, PRO_GN, PRO_GN_SILU = 0, 1, 2
RES_NONE, RES_DOWN, RES_UP, RES_SUBPIX = 0, 1, 2, 3
OUT_NHWC, OUT_QKV, OUT_QV = 0, 1, 4
K_GENERIC, K_WS, K_X3WS = 1, 2, 3
KERNEL_NAME = {K_GENERIC: "conv_fused_kernel", K_WS: "conv3_ws_kernel", K_X3WS: "conv3_x3ws_kernel"}
MODES = (0, 1, 2)
MODE_NAME = {0: "fp32", 1: "bf16", 2: "bf16x3"}
SQRT_HALF = float(torch.tensor(0.5, dtype=torch.float32).sqrt())  # block_kwargs.skip_scale as the engine passes it
GN_EPS = 1e-6
FWD_TOL_X3 = 2e-5         # the bf16x3 forward tolerance the mean-offset cases are read against

MUTANTS = ("replicate_pad", "tap_flip", "concat_shift32", "up_index", "down_three", "rshift_none", "temb_image0", "scale_before_resid",
           "pair_halo", "subpix_phase_swap", "vt_untransposed", "qkv_no_deinterleave", "slot_dropped", "stats_image0", "straddle_octet_g0",
           "no_eps", "softmax_no_scale", "merged_no_wkbq")


def storage(mode):
    return 1 if mode == 1 else 0


def to_storage(t, mode):
    """fp64 values a tensor of the mode's storage type holds exactly."""
    return bf16_round(t) if mode == 1 else t.to(torch.float32).to(F64)


def f32r(t):
    return t.to(torch.float32).to(F64)


def _mag_conv(x, w):
    """conv2d of non-negative operands for a bound: fp32 arithmetic (ten times faster), rounded up."""
    return F.conv2d(x.to(torch.float32), w.to(torch.float32)).to(F64) * (1.0 + 2.0 ** -10)


def sum_rel(n, mode):
    """Relative weight of sum|terms| in the error of an n-term product sum in this mode."""
    return X3 + U * (3 * n + 2) if mode == 2 else U * (n + 2)


# ---- stages shared by the conv, the pool and the head ----------------------------------------------------------------------------------

def pro_stage(x, ab, pro):
    """x [B, H, W, C], ab [B, C, 2] -> (a x + b or its SiLU, error); one fma, then x * sigmoid."""
    if pro == PRO_NONE:
        return x, torch.zeros_like(x)
    a, b = ab[:, None, None, :, 0], ab[:, None, None, :, 1]
    y = a * x + b
    dy = U * y.abs()
    if pro == PRO_GN:
        return y, dy
    s = torch.sigmoid(y)
    t = y * s
    return t, s * (1 + y.abs() * (1 - s)) * dy + y.abs() * _sigmoid_err(y, s) + 2 * U * t.abs() + TINY


def resample(t, dt, res, mut=None):
    if res == RES_NONE:
        return t, dt
    if res == RES_DOWN:
        sl = [(slice(None), slice(i, None, 2), slice(j, None, 2)) for i in (0, 1) for j in (0, 1)]
        if mut == "down_three":
            return 0.25 * sum(t[s] for s in sl[:3]), dt[sl[0]]
        return 0.25 * sum(t[s] for s in sl), 0.25 * (sum(dt[s] for s in sl) + 5 * U * sum(t[s].abs() for s in sl))
    H = 2 * t.shape[1]
    idx = torch.arange(H) >> 1
    if mut == "up_index":
        idx = ((torch.arange(H) + 1) >> 1).clamp(max=H // 2 - 1)
    return t[:, idx][:, :, idx], dt[:, idx][:, :, idx]


def round_operand(t, dt, mode):
    """The operand as the matrix cores get it: rounded to bf16 in mode 1, fp32 otherwise (the bf16x3 split is charged per product)."""
    if mode == 1:
        return stored(t, dt, 1)
    return t, torch.where(dt > 0, dt + U * t.abs(), dt)


def conv_core(op, dop, w, mode, mut=None, extra_rel=0.0):
    """op, dop [B, H, W, Cin] (unpadded), w [Cout, Cin, ks, ks] -> (acc [B, H, W, Cout], error): zero padding, fp64 conv2d."""
    ks = w.shape[-1]
    p = ks // 2
    if mode == 1:
        w = bf16_round(w)
    if mut == "tap_flip":
        w = w.flip(-1, -2)
    x, dx = op.permute(0, 3, 1, 2), dop.permute(0, 3, 1, 2)
    if p:
        xp = F.pad(x, (p, p, p, p), mode="replicate" if mut == "replicate_pad" else "constant")
        if mut == "pair_halo":  # two 8x8 images of a tile stacked with ONE halo row between them
            nodd = xp[1::2].shape[0]
            xp[1::2, :, 0, p:-p] = x[0::2][:nodd, :, -1, :]
        dx = F.pad(dx, (p, p, p, p))
    else:
        xp = x
    acc = F.conv2d(xp, w)
    n = w.shape[1] * ks * ks
    err = _mag_conv(dx, w.abs()) + (sum_rel(n, mode) + extra_rel) * _mag_conv(xp.abs(), w.abs())
    return acc.permute(0, 2, 3, 1), err.permute(0, 2, 3, 1)


def concat(d, mut=None):
    x = d["src1"] if d.get("src2") is None else torch.cat([d["src1"], d["src2"]], -1)
    if mut == "concat_shift32" and d.get("src2") is not None:  # the kernel believing C1 is one 32-channel step shorter
        c1 = d["src1"].shape[-1]
        x = torch.cat([d["src1"][..., : c1 - 32], d["src2"][..., :32], d["src2"]], -1)
    return x


def conv_acc(d, mode, mut=None):
    """The accumulator of a conv case (before the epilogue): (acc, error), NHWC.  Kept apart so that cases which differ only in the
    epilogue (bias of the mean-offset cases, the wrap cases' cycled images) share one fp64 convolution."""
    x = concat(d, mut)
    t, dt = pro_stage(x, d.get("ab"), d["pro"])
    t, dt = resample(t, dt, d["res"], mut)
    op, dop = round_operand(t, dt, mode)
    # RES_SUBPIX multiplies with per-phase sums of up to four weights, formed in fp32 at pack time: three roundings of the merged weight
    return conv_core(op, dop, d["w"], mode, mut, extra_rel=3 * U if d["res"] == RES_SUBPIX else 0.0)


def conv_epilogue(acc, dacc, d, mode, mut=None):
    """-> {"out": (v, bound)} (OUT_NHWC) or {"q", "k", "vt"} / {"q", "vt"}: (acc + bias + temb[n] + resid) * scale, stored."""
    B, H, W, Cout = acc.shape
    st = storage(mode)
    zero = torch.zeros((), dtype=F64)
    bias = d["bias"] if d.get("bias") is not None else zero
    if d["outmode"] != OUT_NHWC:
        v = acc + bias
        err = dacc + 2 * U * (acc.abs() + bias.abs())
        planes = v.reshape(B, H * W, Cout // 256, 256).unbind(2)
        eplanes = err.reshape(B, H * W, Cout // 256, 256).unbind(2)
        names = ("q", "k", "vt") if d["outmode"] == OUT_QKV else ("q", "vt")
        out = {}
        for name, pv, pe in zip(names, planes, eplanes):
            if name == "vt":
                pv, pe = pv.transpose(1, 2), pe.transpose(1, 2)
                if mut == "vt_untransposed":
                    pv = pv.transpose(1, 2).reshape(pv.shape)
            out[name] = (pv, final(pv, pe, st))
        return out
    temb = d["temb"][:, None, None, :] if d.get("temb") is not None else zero
    if mut == "temb_image0" and d.get("temb") is not None:
        temb = d["temb"][:1, None, None, :]
    resid = zero
    if d.get("resid") is not None:
        resid = d["resid"]
        if d.get("rshift"):
            idx = torch.arange(H) >> 1
            if mut == "rshift_none":  # the half-resolution tensor read with the full-resolution index
                idx = torch.arange(H) % (H // 2)
            resid = resid[:, idx][:, :, idx]
    sc = d.get("scale", 1.0)
    if mut == "scale_before_resid":
        v = (acc + bias + temb) * sc + resid
    else:
        v = (acc + bias + temb + resid) * sc
    mag = acc.abs() + bias.abs() + temb.abs() + resid.abs()
    err = abs(sc) * dacc + 5 * U * abs(sc) * mag + U * v.abs()
    if mut == "subpix_phase_swap":
        v = v.clone()
        a, b = v[:, 0::2, 1::2].clone(), v[:, 1::2, 0::2].clone()
        v[:, 0::2, 1::2], v[:, 1::2, 0::2] = b, a
    return {"out": (v, final(v, err, st))}


def qkv_weight(w_ref, mut=None):
    """The q | k | v de-interleave of the 1x1 qkv weights (EDM/network.py:290-294): packed row plane * C + c <- reference row 3 c + plane."""
    if mut == "qkv_no_deinterleave":
        return w_ref
    return torch.cat([w_ref[0::3], w_ref[1::3], w_ref[2::3]], 0)


def conv(d, mode, mut=None):
    dd = d if not d.get("qkv_perm") else dict(d, w=qkv_weight(d["w"], mut))
    acc, dacc = conv_acc(dd, mode, mut)
    return conv_epilogue(acc, dacc, d, mode, mut)


# ---- GroupNorm partial statistics ----------------------------------------------------------------------------------------------------

def slot_map(layout, H):
    """Which statistics slot of its image an output pixel (y, x) of an H x H tensor belongs to -> ([H, H] slot ids, slots per image).
    tile: one slot per 8 x 16 pixel tile, a whole image at 8 x 8 (conv.hip, conv_ws.hip).  x3: one per (tile, producer wave) = two rows of
    a tile, of the image at 8 x 8 (conv_ws3.hip).  x3sub: tiles are cut from the half-resolution source and every (source tile, phase
    2 py + px, producer wave) has a slot holding output pixels (2 y + py, 2 x + px).  rows32: 32 consecutive pixels (stem, merged attention)."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(H), indexing="ij")
    if layout == "tile":
        if H == 8:
            return torch.zeros_like(y), 1
        return (y // 8) * (H // 16) + x // 16, (H // 8) * (H // 16)
    if layout == "x3":
        if H == 8:
            return y // 2, 4
        return ((y // 8) * (H // 16) + x // 16) * 4 + (y % 8) // 2, (H // 8) * (H // 16) * 4
    if layout == "x3sub":
        s, sy, sx, ph = H // 2, y // 2, x // 2, (y % 2) * 2 + (x % 2)
        if s == 8:
            return ph * 4 + sy // 2, 16
        return (((sy // 8) * (s // 16) + sx // 16) * 4 + ph) * 4 + (sy % 8) // 2, (s // 8) * (s // 16) * 16
    assert layout == "rows32"
    return (y * H + x) // 32, H * H // 32


def stats_layout(kernel, res):
    if kernel == K_X3WS:
        return "x3sub" if res == RES_SUBPIX else "x3"
    return "tile"


def slot_stats(v, layout, mut=None):
    """v [B, H, H, C]: the tensor AS STORED -> (stats [B, S, C / 4, 2] = exact {sum, sum of squares} per slot and channel quad, bound):
    the kernels add n = 4 * pixels values (and their squares, each rounded) in fp32, in any order."""
    B, H, _, C = v.shape
    ids, S = slot_map(layout, H)
    onehot = F.one_hot(ids.reshape(-1), S).to(F64)  # [HW, S]
    q = v.reshape(B, H * H, C // 4, 4)
    s1, s2, sa = (torch.einsum("ps,bpq->bsq", onehot, t.sum(-1)) for t in (q, q * q, q.abs()))
    n = 4 * onehot.sum(0).max().item()
    val = torch.stack([s1, s2], -1)
    bound = torch.stack([U * (n + 2) * sa, U * (n + 3) * s2], -1)
    if mut == "slot_dropped":
        val = val.clone()
        val[:, S - 1] = 0
    if mut == "stats_image0":
        val = val[:1].expand_as(val)
    return val, bound


def gn_finalize(st1, st2, gamma, beta, eps, hw, dst1=None, dst2=None, mut=None):
    """gn_finalize_kernel: slots st1 [B, S1, C1 / 4, 2] (| st2) of the virtual concat -> ab [B, C, 2] = {rstd gamma, beta - a mean},
    mr [B, G, 2] = {mean, rstd}: slots and quads combined in fp64, var = sum v^2 / cnt - mean^2 (clamped at 0), mean and rstd rounded to
    fp32.  dst1 / dst2: error bounds of the slots themselves (None: the slots are exact inputs), carried through.  Returns a dict of
    (value, bound) for "ab" and "mr" plus the fp64 per-channel pieces "mean", "dmean", "a", "da" the normalised-value bound needs."""
    parts = [(st1, dst1)] + ([(st2, dst2)] if st2 is not None else [])
    quads = torch.cat([s.sum(1) for s, _ in parts], 1)  # [B, Q, 2]
    mags = torch.cat([s.abs().sum(1) for s, _ in parts], 1)
    dq = torch.cat([(ds.sum(1) if ds is not None else torch.zeros_like(s.sum(1))) for s, ds in parts], 1) + E64 * mags
    B, Q, _ = quads.shape
    C = 4 * Q
    G, cpg = gn_geometry(C)
    grp = lambda t: t.reshape(B, G, cpg // 4, 2).sum(2)
    S, dS = grp(quads), grp(dq)
    cnt = float(cpg * hw)
    mean, ex2 = S[..., 0] / cnt, S[..., 1] / cnt
    var = (ex2 - mean * mean).clamp_min(0.0)
    # the cancellation, explicitly: what sum v^2 / cnt - mean^2 may be off by, against var + eps
    dmean64 = dS[..., 0] / cnt
    dvar = dS[..., 1] / cnt + 2 * mean.abs() * dmean64 + dmean64 ** 2 + E64 * (ex2 + mean * mean)
    ve = var + (0.0 if mut == "no_eps" else eps)
    rstd = ve ** -0.5
    shrink = 1.0 - dvar / ve
    rho = torch.where(shrink > 0, shrink.clamp_min(1e-300) ** -0.5 - 1.0, torch.full_like(shrink, float("inf"))) + 2 * U
    dmean = dmean64 + U * mean.abs()
    if mut == "stats_image0":
        mean, rstd = mean[:1].expand(B, G), rstd[:1].expand(B, G)
    chan = torch.arange(C)
    gidx = chan // cpg
    if mut == "straddle_octet_g0":  # every channel of an octet taking the group of the octet's first channel
        gidx = (chan // 8 * 8) // cpg
    ch = lambda t: t[:, gidx]
    a = ch(rstd) * gamma
    b = beta - a * ch(mean)
    da = a.abs() * (ch(rho) + U)
    db = ch(mean).abs() * da + a.abs() * ch(dmean) + U * (b.abs() + (a * ch(mean)).abs())
    return dict(ab=(torch.stack([a, b], -1), torch.stack([da, db], -1)),
                mr=(torch.stack([mean, rstd], -1), torch.stack([dmean, rstd * (rho + U)], -1)),
                mean=ch(mean), dmean=ch(dmean), a=a, da=da, b=b)


def normalised_bound(x, k):
    """Bound of the normalised value a x + b = a (x - mean) + beta under the coefficient errors of gn_finalize (its dict k), x
    [B, H, W, C]: the errors of a and b are one error of rstd and one of the mean, so |x - mean| da + |a| dmean - not |x| da + db - plus
    the roundings of b and of the fma."""
    e = lambda t: t[:, None, None, :]
    y = e(k["a"]) * x + e(k["b"])
    return (x - e(k["mean"])).abs() * e(k["da"]) + e(k["a"]).abs() * e(k["dmean"]) + U * (e(k["b"]).abs() + e(k["a"] * k["mean"]).abs()) + U * y.abs()


def gn_coeffs_exact(v, gamma, beta, eps):
    """The GroupNorm coefficients of the tensor v [B, H, W, C] itself, two-pass in fp64: {"a", "b"} [B, C]."""
    B, H, W, C = v.shape
    G, cpg = gn_geometry(C)
    vg = v.reshape(B, H * W, G, cpg)
    mean = vg.mean((1, 3))
    var = ((vg - mean[:, None, :, None]) ** 2).mean((1, 3))
    rstd = (var + eps) ** -0.5
    a = rstd.repeat_interleave(cpg, 1) * gamma
    return dict(a=a, b=beta - a * mean.repeat_interleave(cpg, 1), mean=mean, std=var.sqrt())


def gn_silu_pool(x, ab, mode):
    """gn_silu_pool_kernel: out = mean of 2x2 of silu(a x + b), stored."""
    t, dt = pro_stage(x, ab, PRO_GN_SILU)
    t, dt = resample(t, dt, RES_DOWN)
    return t, final(t, dt + U * t.abs(), storage(mode))


# ---- attention -----------------------------------------------------------------------------------------------------------------------

def _softmax(s, ds):
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    P = e / e.sum(-1, keepdim=True)
    dsm = ds.amax(-1, keepdim=True)  # the row maximum carries its own logit's error
    dP = P * (ds + dsm + (P * (ds + dsm)).sum(-1, keepdim=True) + 2 * U * (s - m).abs() + 16 * U) + TINY
    return P, dP


def attention(q, k, vt, mode, mut=None):
    """attention kernels of attn.hip: q, k [B, T, 256], vt [B, 256, T] -> out [B, T, 256] = softmax(q k^T / 16) v; the normalised P is
    the A operand of the second product, so mode 1 rounds it to bf16."""
    T, C = q.shape[-2], q.shape[-1]
    sc = 1.0 if mut == "softmax_no_scale" else 0.0625
    s = sc * (q @ k.transpose(-1, -2))
    ds = sc * sum_rel(C, mode) * (q.abs() @ k.abs().transpose(-1, -2)) + 2 * U * s.abs()
    P, dP = _softmax(s, ds)
    P, dP = stored(P, dP, 1) if mode == 1 else (P, dP + U * P)
    v = vt.transpose(-1, -2)
    o = P @ v
    err = dP @ v.abs() + sum_rel(T, mode) * (P @ v.abs())
    return o, final(o, err, storage(mode))


def attn_merge_weights(qkv_w, qkv_b, proj_w, mut=None):
    """attn_merge_weights_kernel: w_out [2 C][C] = [Wk^T Wq ; Wp Wv], b_out [2 C] = [Wk^T bq ; Wp bv], fp64 sums, one rounding to fp32."""
    Wq, Wk, Wv = qkv_w[0::3], qkv_w[1::3], qkv_w[2::3]
    bq, bv = qkv_b[0::3], qkv_b[2::3]
    C = Wq.shape[0]
    w = torch.cat([Wk.t() @ Wq, proj_w @ Wv], 0)
    b = torch.cat([Wk.t() @ bq, proj_w @ bv], 0)
    if mut == "merged_no_wkbq":
        b = torch.cat([torch.zeros(C, dtype=F64), proj_w @ bv], 0)
    mw = torch.cat([Wk.t().abs() @ Wq.abs(), proj_w.abs() @ Wv.abs()], 0)
    mb = torch.cat([Wk.t().abs() @ bq.abs(), proj_w.abs() @ bv.abs()], 0)
    return (w, U * w.abs() + E64 * C * mw), (b, U * b.abs() + E64 * C * mb)


def attention_merged(qm, x_mid, ab, vmt, bp, scale):
    """attention_x3_lds_kernel<MRG>: out = (softmax(qm xn^T / 16) vm + bp + x_mid) * scale, xn = a x_mid + b (bf16x3 products, fp32 tensors)."""
    T, C = qm.shape[-2], qm.shape[-1]
    a, b = ab[:, None, :, 0], ab[:, None, :, 1]
    xn = a * x_mid + b
    dxn = U * xn.abs()
    s = 0.0625 * (qm @ xn.transpose(-1, -2))
    ds = 0.0625 * (qm.abs() @ dxn.transpose(-1, -2) + sum_rel(C, 2) * (qm.abs() @ xn.abs().transpose(-1, -2))) + 2 * U * s.abs()
    P, dP = _softmax(s, ds)
    dP = dP + U * P
    vm = vmt.transpose(-1, -2)
    o = P @ vm
    do = dP @ vm.abs() + sum_rel(T, 2) * (P @ vm.abs())
    v = (o + bp + x_mid) * scale
    err = abs(scale) * do + 5 * U * abs(scale) * (o.abs() + bp.abs() + x_mid.abs()) + U * v.abs()
    return v, final(v, err, 0)


# ---- stem and output head --------------------------------------------------------------------------------------------------------------

def stem(x, c_in, w, bias, mode, mfma):
    """out NHWC = conv3x3(c_in[n] x) + bias, x NCHW fp32.  mfma (stem_kernel): the operand and the weights in the storage type (bf16 in
    mode 1, else exact fp32 products); else conv_in_kernel: fp32 fma arithmetic in every mode.  Stored in the storage type."""
    v = (c_in[:, None, None, None] * x).permute(0, 2, 3, 1)
    dv = U * v.abs()
    arith = 1 if (mfma and mode == 1) else 0
    op, dop = round_operand(v, dv, arith)
    acc, dacc = conv_core(op, dop, w, arith)
    out = acc + bias
    return out, final(out, dacc + 2 * U * (acc.abs() + bias.abs()), storage(mode))


def aux(x, ab, w, bias, x_t, coef, mode, mfma):
    """D NCHW fp32 = c_skip[n] x_t + c_out[n] (conv3x3(silu(a x + b)) + bias).  mfma (aux_head_kernel): the products of the compute
    mode; else aux_out_kernel: fp32 fma arithmetic on the storage-type x."""
    B = x.shape[0]
    t, dt = pro_stage(x, ab, PRO_GN_SILU)
    arith = mode if mfma else 0
    op, dop = round_operand(t, dt, arith)
    acc, dacc = conv_core(op, dop, w, arith)
    Fv = (acc + bias).permute(0, 3, 1, 2)
    dF = (dacc + 2 * U * (acc.abs() + bias.abs())).permute(0, 3, 1, 2)
    cs, co = coef[2 * B:3 * B][:, None, None, None], coef[3 * B:4 * B][:, None, None, None]
    D = cs * x_t + co * Fv
    return D, co.abs() * dF + 3 * U * ((cs * x_t).abs() + (co * Fv).abs()) + U * D.abs()


def edm_coef(t, sigma_data=0.5):
    """coef [5][B] = c_in, c_noise, c_skip, c_out, r_noise of EDM's preconditioning at the times t (fp32 values, an INPUT of the ops)."""
    t = torch.as_tensor(t, dtype=F64)
    sd2 = sigma_data ** 2
    rows = [1 / (sd2 + t * t).sqrt(), t.log() / 4, sd2 / (t * t + sd2), t * sigma_data / (t * t + sd2).sqrt(), torch.zeros_like(t)]
    return f32r(torch.cat(rows))


# ---- the designed inputs -----------------------------------------------------------------------------------------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def bordered(t, factor=100.0):
    """Border rows and columns of [B, H, W, C] `factor` times the interior: a wrong halo pixel or padding row moves an output far."""
    t = t.clone()
    t[:, 0], t[:, -1] = t[:, 0] * factor, t[:, -1] * factor
    t[:, 1:-1, 0], t[:, 1:-1, -1] = t[:, 1:-1, 0] * factor, t[:, 1:-1, -1] * factor
    return t


def design_ab(B, C, g):
    """a with mixed signs and one zero, the last image's coefficients 1000 x larger (a coefficient row taken from the neighbouring image
    shows)."""
    a = (1.0 + 0.5 * torch.randn(B, C, generator=g, dtype=F64)) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    a[:, 5] = 0.0
    b = 0.3 * torch.randn(B, C, generator=g, dtype=F64)
    if B > 1:
        a[B - 1] *= 1000.0
        b[B - 1] *= 1000.0
    return f32r(torch.stack([a, b], -1))


# name: (ks, pro, res, outmode, c1, c2, h, batch, flags).  flags: t temb, r residual (+ scale sqrt(1/2)), s rshift, q qkv_perm.
# cin 128 = four K steps (the ring minimum); 256 + 128 / 256 + 256: the concat crosses inside / on a K step of 64; 8x8 at batch 3: a
# full image pair and a half-empty one; batch 1, 2, 3 all occur.
CONV_CASES = {
    "c3_128_32_b3": (3, PRO_GN_SILU, RES_NONE, OUT_NHWC, 128, 0, 32, 3, "t"),
    "c3_384_16_b2": (3, PRO_GN_SILU, RES_NONE, OUT_NHWC, 256, 128, 16, 2, "r"),
    "c3_512_8_b3": (3, PRO_GN_SILU, RES_NONE, OUT_NHWC, 256, 256, 8, 3, "tr"),
    "c3_256_16_b3": (3, PRO_GN_SILU, RES_NONE, OUT_NHWC, 256, 0, 16, 3, "t"),
    "c3up_384_32_b1": (3, PRO_GN_SILU, RES_UP, OUT_NHWC, 256, 128, 32, 1, "t"),
    "c3up_512_16_b3": (3, PRO_GN_SILU, RES_UP, OUT_NHWC, 256, 256, 16, 3, "t"),
    "c3raw_256_16_b3": (3, PRO_NONE, RES_NONE, OUT_NHWC, 256, 0, 16, 3, "t"),
    "c3raw_128_8_b2": (3, PRO_NONE, RES_NONE, OUT_NHWC, 128, 0, 8, 2, "t"),
    "c3raw_128_32_b1": (3, PRO_NONE, RES_NONE, OUT_NHWC, 128, 0, 32, 1, ""),
    "c1_128_32_b2": (1, PRO_NONE, RES_NONE, OUT_NHWC, 128, 0, 32, 2, ""),
    "c1_256_8_b3": (1, PRO_NONE, RES_NONE, OUT_NHWC, 256, 0, 8, 3, "r"),
    "c1down_128_16_b3": (1, PRO_NONE, RES_DOWN, OUT_NHWC, 128, 0, 16, 3, ""),
    "c1up_512_16_b1": (1, PRO_NONE, RES_UP, OUT_NHWC, 256, 256, 16, 1, ""),
    "c1up_384_32_b2": (1, PRO_NONE, RES_UP, OUT_NHWC, 256, 128, 32, 2, ""),
    "qkv_16_b3": (1, PRO_GN, RES_NONE, OUT_QKV, 256, 0, 16, 3, "q"),
    "qkv_8_b3": (1, PRO_GN, RES_NONE, OUT_QKV, 256, 0, 8, 3, "q"),
    "qv_16_b2": (1, PRO_GN, RES_NONE, OUT_QV, 256, 0, 16, 2, ""),
    "sub_512_16_b3": (3, PRO_GN_SILU, RES_SUBPIX, OUT_NHWC, 256, 256, 16, 3, "t"),
    "sub_384_32_b2": (3, PRO_GN_SILU, RES_SUBPIX, OUT_NHWC, 256, 128, 32, 2, "t"),
    "rs_256_16_b3": (3, PRO_GN_SILU, RES_NONE, OUT_NHWC, 256, 0, 16, 3, "rs"),
    "rs_256_32_b1": (3, PRO_GN_SILU, RES_NONE, OUT_NHWC, 256, 0, 32, 1, "rs"),
}
# wrap of the persistent kernels: more tiles than CUs; the images are those of the base case, cycled
WRAP_CASES = {"wrap_32": ("c3_128_32_b3", 33), "wrap_16": ("c3_256_16_b3", 129)}


def conv_modes(name):
    """The compute modes whose launch_t / wave-specialised dispatch accepts the case."""
    if name.startswith(("sub_", "rs_", "qv_")):
        return (2,)
    return MODES


def conv_cout(case):
    return {OUT_QKV: 768, OUT_QV: 512}.get(case[3], 256)


def src_res(res, h):
    return 2 * h if res == RES_DOWN else (h // 2 if res in (RES_UP, RES_SUBPIX) else h)


def expected_plan(mode, case):
    """What the headers of conv.h / conv_ws.hip / conv_ws3.hip say the dispatch takes (FASTGEN_AMD_CONV_WS unset)."""
    ks, pro, res, outmode, c1, c2, h, B, flags = case
    cin = c1 + c2
    tile = {32: 8, 16: 2, 8: 1}[h]
    if ks == 3 and outmode == OUT_NHWC:
        if mode == 1 and h in (16, 32) and ((pro == PRO_GN_SILU and res in (RES_NONE, RES_UP) and (cin >= 256 or (res == RES_NONE and h == 32)))
                                            or (pro == PRO_NONE and cin >= 256)):
            return K_WS, tile
        if mode == 2 and res == RES_SUBPIX:
            return K_X3WS, {16: 2, 8: 1}[h // 2] * 16
        if mode == 2 and (h > 8 or res == RES_NONE):
            return K_X3WS, (tile if h > 8 else 1) * 4
    return K_GENERIC, tile


OFFSET_BASE = "c3_128_32_b3"  # 32x32, 256 output channels = 8 per group, 128-pixel slots: the shape of the CPU model in DESIGN.md


def offset_case(mode, offset, base):
    """The mean-offset cases: OFFSET_BASE with temb[n] raised by offset * (the std of the un-shifted output's group), so that the stored
    tensor has per-group mean / std = offset in every image.  base = (inputs, acc, dacc) of OFFSET_BASE, computed once.  Returns the
    shifted inputs, acc, dacc and the next norm's gamma, beta."""
    d, acc, dacc = base
    v0 = conv_epilogue(acc, dacc, d, mode)["out"][0]
    G, cpg = gn_geometry(d["cout"])
    std = v0.reshape(d["B"], -1, G, cpg).std((1, 3), unbiased=False).repeat_interleave(cpg, 1)
    g = _gen(8000)
    gamma = f32r(1.0 + 0.5 * torch.randn(d["cout"], generator=g, dtype=F64))
    beta = f32r(0.3 * torch.randn(d["cout"], generator=g, dtype=F64))
    return dict(d, temb=f32r(d["temb"] + offset * std)), acc, dacc, gamma, beta


def conv_inputs(name, mode, batch=None):
    """The designed inputs of a conv case in `mode` (values exact in the storage type / fp32): borders 100 x the interior, designed ab,
    temb and bias of the size of the result, the residual with scale sqrt(1/2)."""
    ks, pro, res, outmode, c1, c2, h, B, flags = CONV_CASES[name]
    B = batch or B
    g = _gen(3000 + sum(map(ord, name)))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    # cubed deviates (E z^6 = 15) for activations and weights: a few large terms carry each dot product, so sum|terms| / |sum| - and
    # with it u (n + 2) sum|terms| against the result - stays small at the 4608 terms of a 512-channel 3x3 conv
    rc = lambda *s: torch.randn(*s, generator=g, dtype=F64) ** 3 / math.sqrt(15.0)
    hs, cin, cout = src_res(res, h), c1 + c2, conv_cout(CONV_CASES[name])
    d = dict(name=name, ks=ks, pro=pro, res=res, outmode=outmode, c1=c1, c2=c2, h=h, hs=hs, B=B, cout=cout, qkv_perm="q" in flags,
             rshift=1 if "s" in flags else 0)
    d["src1"] = to_storage(bordered(rc(B, hs, hs, c1)), mode)
    d["src2"] = to_storage(bordered(rc(B, hs, hs, c2)), mode) if c2 else None
    d["ab"] = design_ab(B, cin, g) if pro != PRO_NONE else None
    d["w"] = f32r(rc(cout, cin, ks, ks) / math.sqrt(cin * ks * ks))
    d["bias"] = f32r(rn(cout))
    d["temb"] = f32r(rn(B, cout) * (1.0 + 9.0 * torch.arange(B, dtype=F64)[:, None])) if "t" in flags else None
    if "r" in flags:
        hr = h // 2 if "s" in flags else h
        d["resid"] = to_storage(bordered(rn(B, hr, hr, cout)), mode)
        d["scale"] = SQRT_HALF
    else:
        d["resid"], d["scale"] = None, 1.0
    return d


def cycle_images(d, batch):
    """The wrap cases: a case's images (and per-image rows) repeated up to `batch`."""
    idx = torch.arange(batch) % d["B"]
    out = dict(d, B=batch)
    for key in ("src1", "src2", "ab", "temb", "resid"):
        if d.get(key) is not None:
            out[key] = d[key][idx]
    return out, idx


ATTN_CASES = [(T, B, fam) for T in (64, 256) for B, fam in ((1, "noise"), (3, "eqkeys"), (1, "q0"), (3, "peaked"))]


def attn_inputs(case, mode):
    """q, k [B, T, 256], vt [B, 256, T].  noise: seeded (cubed deviates: a few large terms carry each dot product); q0: q = 0, P uniform;
    peaked: rows 0, 4, .. peak at key 0 and rows 2, 6, .. at key T - 1; eqkeys: the last image has all-equal keys."""
    T, B, fam = case
    C = 256
    g = _gen(4000 + T + 7 * B + sum(map(ord, fam)))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64) ** 3
    q, k, vt = rn(B, T, C) / 15.0, rn(B, T, C), rn(B, C, T)  # E z^6 = 15: logits of unit variance
    if fam == "q0":
        q = torch.zeros_like(q)
    elif fam == "peaked":
        dvec = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).to(F64)
        i = torch.arange(T)
        sign = torch.where(i % 4 == 0, 1.0, torch.where(i % 4 == 2, -1.0, 0.0)).to(F64)[None, :, None]
        q = 8.0 * (0.1 * q + sign * dvec * 16.0 / C)
        k = 0.25 * k
        k[:, 0], k[:, T - 1] = dvec, -dvec
    elif fam == "eqkeys":
        k[B - 1] = k[B - 1, :1]
    return dict(q=to_storage(q, mode), k=to_storage(k, mode), vt=to_storage(vt, mode))


def merged_inputs(B, seed=0):
    """The merged attention block at C = 256, T = 256: reference-layout qkv / proj parameters with N(0, 1) biases, x_mid and norm2 coefficients."""
    C, T = 256, 256
    g = _gen(5000 + B + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    rc = lambda *s: torch.randn(*s, generator=g, dtype=F64) ** 3 / math.sqrt(15.0)  # cubed deviates, as conv_inputs
    d = dict(qkv_w=f32r(rc(3 * C, C) / math.sqrt(C)), qkv_b=f32r(rn(3 * C)), proj_w=f32r(rc(C, C) / math.sqrt(C)), proj_b=f32r(rn(C)),
             x_mid=f32r(rc(B, T, C) + 0.25 * rn(1, 1, C)))
    a = (1.0 + 0.5 * rn(B, C)) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    a[:, 5] = 0.0
    d["ab"] = f32r(torch.stack([a, 0.3 * rn(B, C)], -1))
    return d


# synthetic slots of gn_finalize: (c1, s1, c2, s2, batch), the slot counts of the producing kernels (8 / 2 / 1 tiles, 32 / 8 / 4 of
# conv_ws3.hip, its 32-slot RES_SUBPIX form, the stem's 32, the merged attention's 8); two producers with different counts; cpg 4, 8, 12, 16
GN_SYNTH = [(128, 32, 0, 0, 1), (256, 8, 0, 0, 3), (256, 32, 128, 8, 3), (256, 4, 256, 1, 1), (256, 2, 128, 32, 1), (256, 8, 256, 16, 3)]
GN_OFFSETS = (0, 1, 4, 16, 64)


def gn_synth_inputs(case, offset, hw=1024):
    """Slots as a producer would leave them for a tensor of per-group mean / std = offset: fp32 values of exact partial sums of seeded
    data (a slot = hw / S pixels), one group of tiny variance (eps matters there), gamma with mixed signs and a zero."""
    c1, s1, c2, s2, B = case
    C = c1 + c2
    G, cpg = gn_geometry(C)
    g = _gen(6000 + C + s1 + 3 * s2 + B + 11 * offset)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x = rn(B, hw, C) + float(offset) + 0.25 * rn(1, 1, C)
    x[:, :, cpg:2 * cpg] = 3.0 + 1e-3 * rn(B, hw, cpg)  # group 1: variance 1e-6, the size of eps
    if B > 1:
        x[B - 1] *= 1000.0
    x = f32r(x)
    def slots(v, S):
        q = v.reshape(B, S, hw // S, v.shape[-1] // 4, 4)
        return f32r(torch.stack([q.sum((2, 4)), (q * q).sum((2, 4))], -1))
    gamma = (1.0 + 0.5 * rn(C)) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    gamma[C // 2 + 1] = 0.0
    return dict(st1=slots(x[..., :c1], s1), st2=slots(x[..., c1:], s2) if c2 else None, gamma=f32r(gamma), beta=f32r(0.3 * rn(C)), hw=hw, x=x)
