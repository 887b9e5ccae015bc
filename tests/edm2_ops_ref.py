"""fp64 references of the EDM2 kernels and of the shared linear, one per test-only entry point (fg_op_adm_conv_ex, fg_op_edm2_attention,
fg_op_edm2_prep_weight, fg_op_edm2_pixel_norm, fg_op_linear), the designed inputs and the error bounds of tests/test_gpu_edm2_ops.py, and
for every reference a set of MUTANTS: the same operation with one plausible kernel error.  tests/test_edm2_ops_ref.py shows on the CPU
that each bound passes the fp32 oracle and separates every mutant by 5x or more on the GPU test's own inputs.  CPU only, plain torch."""
import math

import torch
import torch.nn.functional as F

from test_gpu_adm_ops import attention_inputs, conv_case_ref, conv_prologue, mean2x2  # noqa: F401  (plain torch helpers, no GPU)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ratio(err, bound):
    """max err / bound; 0 / 0 counts as 0 (an exact value met exactly), anything non-finite or x / 0 as inf."""
    err, bound = err.double(), bound.double().expand_as(err)
    r = torch.where((err == 0) & (bound == 0), torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return r.max().item()


# ---- convolution with ab_stride, resid_scale and clip ---------------------------------------------------------------------------
# ab: "ones" the {1, 0} row and "cat" the mp_cat row {wa .. | wb .., 0}, both read with ab_stride 0; "strided" rows of a [B, stride]
# matrix from channel offset `off`, as conv_res1 reads the stacked modulation; "dense" [B, C] rows with ab_stride -1 (with resid_scale 1
# and clip 0: the call fg_op_adm_conv makes); None no prologue.  The buffer the kernel gets
# (conv_ab_buffer) holds junk wherever the kernel must not read: a broadcast row is followed by B - 1 junk rows.
CONV_EX_CASES = {
    "bcast_ones": dict(ks=3, C1=64, C2=0, cout=64, H=8, B=3, res_mode=0, ab="ones", silu=1, resid_mode=None, resid_scale=1.0, clip=0.0),
    "bcast_cat": dict(ks=3, C1=96, C2=32, cout=64, H=8, B=3, res_mode=0, ab="cat", silu=1, resid_mode=None, resid_scale=1.0, clip=0.0),
    "strided": dict(ks=3, C1=64, C2=0, cout=64, H=8, B=3, res_mode=0, ab="strided", silu=1, resid_mode=None, resid_scale=1.0, clip=0.0),
    "up": dict(ks=3, C1=64, C2=0, cout=64, H=16, B=3, res_mode=2, ab="ones", silu=1, resid_mode=2, resid_scale=0.9191450, clip=0.0),
    "resid0": dict(ks=3, C1=64, C2=0, cout=96, H=8, B=3, res_mode=0, ab="strided", silu=1, resid_mode=0, resid_scale=0.9191450, clip=0.0),
    "clip": dict(ks=1, C1=64, C2=0, cout=64, H=8, B=3, res_mode=0, ab=None, silu=0, resid_mode=0, resid_scale=0.9191450, clip=256.0),
    "dense": dict(ks=3, C1=64, C2=0, cout=96, H=8, B=3, res_mode=0, ab="dense", silu=1, resid_mode=0, resid_scale=1.0, clip=0.0),
    "out_conv": dict(ks=3, C1=64, C2=0, cout=3, H=8, B=3, res_mode=0, ab=None, silu=0, resid_mode=None, resid_scale=1.0, clip=0.0),
    "qkv": dict(ks=1, C1=64, C2=0, cout=192, H=8, B=3, res_mode=0, ab=None, silu=0, resid_mode=None, resid_scale=1.0, clip=0.0),
}
AB_STRIDE, AB_OFF = 200, 72
CONV_MUTANTS = {  # mutant -> the cases built to see it
    "ab_image0": ["strided", "resid0"],
    "ab_dense_stride": ["bcast_ones", "bcast_cat", "strided", "resid0"],
    "resid_scale_dropped": ["up", "resid0", "clip"],
    "clip_before_resid": ["clip"],
    "clip_dropped": ["clip"],
}


def conv_ex_inputs(name):
    """x NCHW at the source resolution, the ab buffer [rows, width, 2] (or None) with (ab_stride, first element), w OIHW, resid NCHW."""
    c = CONV_EX_CASES[name]
    g = gen(sum(map(ord, name)))
    B, C, H = c["B"], c["C1"] + c["C2"], c["H"]
    Hs = {0: H, 1: 2 * H, 2: H // 2}[c["res_mode"]]
    big = 300.0 if c["clip"] else 1.0
    x = big * torch.randn(B, C, Hs, Hs, generator=g)
    w = torch.randn(c["cout"], C, c["ks"], c["ks"], generator=g) / math.sqrt(C * c["ks"] ** 2)
    ab, stride, off = None, -1, 0
    if c["ab"] in ("ones", "cat"):
        ab = torch.stack([1 + 0.5 * torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)], dim=-1)  # rows 1 ..: junk
        ab[0, :, 1] = 0
        ab[0, :, 0] = 1.0
        if c["ab"] == "cat":
            ab[0, :c["C1"], 0], ab[0, c["C1"]:, 0] = 0.8164966, 1.4142135
        stride = 0
    elif c["ab"] == "strided":
        ab = torch.stack([1 + 0.5 * torch.randn(B, AB_STRIDE, generator=g), torch.zeros(B, AB_STRIDE)], dim=-1)
        ab[..., 1] = 0.3 * torch.randn(B, AB_STRIDE, generator=g)
        stride, off = AB_STRIDE, AB_OFF
    elif c["ab"] == "dense":
        ab = torch.stack([1 + 0.3 * torch.randn(B, C, generator=g), 0.3 * torch.randn(B, C, generator=g)], dim=-1)
    resid = None
    if c["resid_mode"] is not None:
        R = {0: H, 1: 2 * H, 2: H // 2}[c["resid_mode"]]
        resid = (big if c["clip"] else 4.0) * torch.randn(B, c["cout"], R, R, generator=g)
    return x, ab, stride, off, w, resid


def conv_ab_rows(ab, stride, off, B, C, mutant=None):
    """[B, C, 2]: the rows a kernel reads from the buffer `ab` ([rows, width, 2] flattened) with the given stride and first element."""
    if ab is None:
        return None
    flat = ab.reshape(-1, 2)
    if mutant == "ab_image0":
        step = 0
    elif mutant == "ab_dense_stride" or stride < 0:
        step = C
    else:
        step = stride
    return torch.stack([flat[off + b * step: off + b * step + C] for b in range(B)])


def conv_ex_ref(name, bf16_operands, mutant=None):
    """(fp64 reference, the error bound's magnitude terms (|x'| (*) |w|, |resid_scale * resid|)) of one fg_op_adm_conv_ex case."""
    c = CONV_EX_CASES[name]
    x, ab, stride, off, w, resid = conv_ex_inputs(name)
    rows = conv_ab_rows(ab, stride, off, c["B"], c["C1"] + c["C2"], mutant)
    ref, mag = conv_case_ref(x, rows, c["silu"], c["res_mode"], w, None, None, None, bf16_operands)
    clip = c["clip"]
    if mutant == "clip_before_resid" and clip:
        ref = ref.clamp(-clip, clip)
    sr = torch.zeros_like(ref)
    if resid is not None:
        r = {0: resid, 2: resid.repeat_interleave(2, 2).repeat_interleave(2, 3)}[c["resid_mode"]].double()
        sr = r * (1.0 if mutant == "resid_scale_dropped" else float(torch.tensor(c["resid_scale"]).float()))
        ref = ref + sr
    if clip and mutant not in ("clip_before_resid", "clip_dropped"):
        ref = ref.clamp(-clip, clip)
    return ref, mag, sr.abs()


def conv_ex_bound(name, mode):
    """test_conv's bounds + 2^-22 |resid_scale * resid| (the product's and the sum's roundings); a clamp never enlarges an error."""
    c = CONV_EX_CASES[name]
    _, exact_mag, sr = conv_ex_ref(name, False)
    if mode == "bf16x3":
        return 2.0 ** -15 * exact_mag + 1e-6 + 2.0 ** -22 * sr
    _, mag, _ = conv_ex_ref(name, True)
    return (2.0 ** -17 if c["ab"] is None else 2.0 ** -7) * mag + 2.0 ** -22 * sr


# ---- cosine attention ---------------------------------------------------------------------------------------------------------------
ATTN_SHAPES = [(1, 64, 1), (2, 256, 3), (1, 1024, 6), (1, 64, 12)]  # (B, T, heads)
ATTN_KINDS = ["random", "tiny", "aligned", "uniform"]
ATTN_MUTANTS = ["v_raw", "k_raw", "eps_dropped", "eps_1e-3", "scale_1pc", "neighbour_head"]


def mp_attention_inputs(B, T, heads, kind, seed):
    """q, k, v [B, heads, T, 64].  random / uniform: attention_inputs at logit scale 1 (uniform: every key equal).  tiny: rows scaled
    by 1e-3 and 1e-5, where eps = 1e-4 decides the normalised row (|row| / 8 ~ 1e-3, 1e-5), and an all-zero row, in different places
    of q, k and v.  aligned: the last 32 keys are the first 32 queries plus 2 % noise, so for those queries the running maximum
    moves in the last key tile and the largest logit nears the cosine limit 8."""
    if kind in ("random", "uniform"):
        return attention_inputs(B, T, heads, 1, kind, seed)
    g = gen(seed)
    q, k, v = (torch.randn(B, heads, T, 64, generator=g) for _ in range(3))
    if kind == "tiny":
        for i, t in enumerate((q, k, v)):
            t[:, :, 3 + 7 * i::16] *= 1e-3
            t[:, :, 5 + 3 * i::16] *= 1e-5
            t[:, :, 11 + i] = 0
            t[:, :, T - 2 - i] = 0
    elif kind == "aligned":
        k[:, :, T - 32:] = q[:, :, :32] + 0.02 * torch.randn(B, heads, 32, 64, generator=g)
    else:
        raise ValueError(kind)
    return q, k, v


def mp_normalize(x, eps=1e-4):
    return x / (eps + torch.linalg.vector_norm(x, dim=-1, keepdim=True) / 8)


def mp_attention_ref(q, k, v, mutant=None):
    """softmax_k(q^ . k^ / 8) v^ with x^ = x / (1e-4 + |x| / 8) over the 64 channels, in the dtype of the inputs."""
    eps = {"eps_dropped": 0.0, "eps_1e-3": 1e-3}.get(mutant, 1e-4)
    if mutant == "neighbour_head":  # the norm of head h + 1's rows
        n = lambda x: x / (eps + torch.linalg.vector_norm(x.roll(-1, 1), dim=-1, keepdim=True) / 8)  # noqa: E731
    else:
        n = lambda x: mp_normalize(x, eps)  # noqa: E731
    qn, kn, vn = n(q), (k if mutant == "k_raw" else n(k)), (v if mutant == "v_raw" else n(v))
    scale = 0.125 * (1.01 if mutant == "scale_1pc" else 1.0)
    logits = torch.einsum("bhqc,bhkc->bhqk", qn, kn) * scale
    return torch.einsum("bhqk,bhkc->bhqc", logits.softmax(-1), vn)


ATTN_C0, ATTN_C1 = 4e-6, 1e-6


def mp_attention_bound(q, k, v):
    """test_attention's form on the fp64-normalised tensors: max|v^| (4e-6 + 1e-6 max_k(|q^| . |k^|) / 8) per query."""
    qn, kn, vn = mp_normalize(q.double()), mp_normalize(k.double()), mp_normalize(v.double())
    mag = torch.einsum("bhqc,bhkc->bhqk", qn.abs(), kn.abs()).amax(-1, keepdim=True) / 8
    return vn.abs().amax(dim=(2, 3), keepdim=True) * (ATTN_C0 + ATTN_C1 * mag)


# ---- weight preparation -------------------------------------------------------------------------------------------------------------
# (cout, cin, cin_pad, taps, gain, extra0, extra1, c_split): the stem, the widest fan (9 x 1536 = 13 824), a fan that is no multiple
# of 256, mp_cat's two weights; row 1 of every case is all zero (eps alone).
PREP_CASES = {
    "stem": (64, 4, 32, 9, None, 1.0, 1.0, 32),
    "wide": (64, 1536, 1536, 9, None, 1.6778523, 1.6778523, 1536),
    "wide_gain": (64, 1536, 1536, 9, 0.37, 1.0, 1.0, 1536),
    "fan1000": (128, 1000, 1000, 1, 0.6, 2.3, 1.0, 1000),
    "cat": (64, 96, 96, 1, None, 0.8164966, 1.4142135, 64),
    "cat_gain": (64, 96, 96, 1, 1.7, 0.8164966, 1.4142135, 64),
}
PREP_MUTANTS = {"eps_dropped": list(PREP_CASES), "gain_dropped": ["wide_gain", "fan1000", "cat_gain"], "c_split_off_by_one": ["cat", "cat_gain"],
                "extra1_everywhere": ["cat", "fan1000"], "norm_over_cin_pad": ["stem"]}


def prep_inputs(name):
    cout, cin, cin_pad, taps, gain, e0, e1, c_split = PREP_CASES[name]
    w = torch.randn(cout, cin, taps, generator=gen(cout + cin + taps)) * 1.7
    w[1] = 0
    return w


def prep_weight_ref(name, w, mutant=None):
    """[cout, cin_pad, taps] in w's dtype; the fp32 scalars (gain, extras) enter as their fp32 values."""
    cout, cin, cin_pad, taps, gain, e0, e1, c_split = PREP_CASES[name]
    f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))  # noqa: E731
    fan = (cin_pad if mutant == "norm_over_cin_pad" else cin) * taps
    eps = 0.0 if mutant == "eps_dropped" else 1e-4
    n = torch.linalg.vector_norm(w.reshape(cout, -1), dim=1).reshape(-1, 1, 1)
    g = 1.0 if gain is None or mutant == "gain_dropped" else f32(gain)
    split = c_split - 1 if mutant == "c_split_off_by_one" else c_split
    extra = torch.where(torch.arange(cin) < split, f32(e0), f32(e1)).to(w.dtype).reshape(1, -1, 1)
    if mutant == "extra1_everywhere":
        extra = torch.full_like(extra, f32(e1))
    out = w * extra * (g / math.sqrt(fan)) / (eps + n / math.sqrt(fan))
    return F.pad(out, (0, 0, 0, cin_pad - cin))


PREP_REL = 2.0 ** -18  # the 256-way strided sum of squares plus the tree at fan 13 824, worst case


# ---- pixel norm -----------------------------------------------------------------------------------------------------------------------
PIXNORM_CASES = [(B, H, C, down) for C in (64, 192, 768) for H in (8, 16) for down in (0, 1) for B in (3,)] + [(1, 1, 192, 0), (1, 1, 64, 1)]
PIXNORM_MUTANTS = {"mean_after_norm": 1, "sqrt_c_dropped": None, "eps_dropped": None}  # value: the `down` a mutant needs (None: any)


def pixnorm_inputs(B, H, C, down):
    """NCHW at the source resolution, with one all-zero output pixel (the whole 2x2 window with down) where there is more than one."""
    R = 2 * H if down else H
    x = torch.randn(B, C, R, R, generator=gen(B + H + C + down)) * 2.5
    if B * H * H > 1:
        x[0, :, :2 if down else 1, :2 if down else 1] = 0
    return x


def pixel_norm_ref(x, down, mutant=None):
    """(x or its 2x2 mean) / (1e-4 + |.| / sqrt(C)) over the channels, NCHW; returns (out, the normaliser, the mean |x| of the window)."""
    eps = 0.0 if mutant == "eps_dropped" else 1e-4
    rc = 1.0 if mutant == "sqrt_c_dropped" else math.sqrt(x.shape[1])
    norm = lambda u: 1 / (eps + torch.linalg.vector_norm(u, dim=1, keepdim=True) / rc)  # noqa: E731
    abar = F.avg_pool2d(x.abs(), 2) if down else x.abs()
    if down and mutant == "mean_after_norm":
        return F.avg_pool2d(x * norm(x), 2), None, abar
    m = F.avg_pool2d(x, 2) if down else x
    return m * norm(m), norm(m), abar


PIXNORM_REL = 2.0 ** -20


# ---- linear ---------------------------------------------------------------------------------------------------------------------------
# (arm, B, I, O): every dispatch arm of launch_linear at ragged batches; KB: the k block of the arm
LINEAR_CASES = [("generic", 5, 10, 256), ("generic", 70, 1000, 96), ("kb16", 33, 48, 64), ("kb64", 1, 192, 768), ("kb64", 32, 768, 3392),
                ("pair", 33, 768, 3392), ("pair", 65, 768, 3392), ("pair", 128, 768, 3392)]
LINEAR_KB = {"generic": 16, "kb16": 16, "kb64": 64, "pair": 64}
LINEAR_MUTANTS = ["last_k_block_dropped", "bias_after_silu", "pair_rows_repeated"]


def linear_arm(B, I, O):
    """The arm launch_linear takes (fastgen_amd/csrc/misc.hip)."""
    if I % 16 or O % 32:
        return "generic"
    if I % 64 == 0 and B > 32 and O >= 2048:
        return "pair"
    return "kb64" if I % 64 == 0 else "kb16"


def linear_inputs(B, I, O):
    g = gen(B + I + O)
    return torch.randn(B, I, generator=g), torch.randn(O, I, generator=g) / math.sqrt(I), 0.5 * torch.randn(O, generator=g)


def linear_ref(x, w, bias, silu, mutant=None, kb=16):
    """(act(x w^T + bias), the bound before the activation: in 2^-24 |x| |w|^T + 2^-23 |bias|), in x's dtype."""
    I = x.shape[1]
    if mutant == "last_k_block_dropped":
        keep = (I - 1) // kb * kb
        x = torch.cat([x[:, :keep], torch.zeros_like(x[:, keep:])], 1)
    y = x @ w.t()
    bound = I * 2.0 ** -24 * (x.abs() @ w.abs().t())
    if bias is not None:
        bound = bound + 2.0 ** -23 * bias.abs()
    if mutant == "bias_after_silu" and silu and bias is not None:
        y = F.silu(y) + bias
    else:
        y = y if bias is None else y + bias
        y = F.silu(y) if silu else y
    if mutant == "pair_rows_repeated":  # rows 32 .. 63 of every 64-row tile computed from the x rows of 0 .. 31
        y = y.clone()
        for b0 in range(0, y.shape[0], 64):
            n = max(0, min(64, y.shape[0] - b0) - 32)
            y[b0 + 32: b0 + 32 + n] = y[b0: b0 + n]
    return y, bound * (1.1 if silu else 1.0)  # SiLU is 1.1-Lipschitz


# ---- blocks and the network in fp64 -----------------------------------------------------------------------------------------------------
BLOCK_MAX_REL = 2e-5   # bf16x3: max|d| / max|ref| per block, as test_gpu_adm_ops.test_blocks_narrow
BLOCK_REL_L2 = 5e-3    # bf16: relative L2 per block


class to64(dict):
    """A state dict read in fp64, entry by entry (no second copy of a 280 M parameter network)."""

    def __getitem__(self, key):
        return dict.__getitem__(self, key).double()
