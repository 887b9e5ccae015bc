"""fp64 references of the EDM2 tangent kernels (fg_op_edm2_attention_jvp, fg_op_edm2_pixel_norm_jvp, fg_op_edm2_silu_operand_jvp,
fg_edm2_run_block_jvp, fg_edm2_jvp), each written as torch.func.jvp of the corresponding function of tests/edm2_ops_ref.py or
tests/edm2_ref.py; the same derivatives as closed formulas (what the kernels compute; evaluated in fp32 they are the CPU oracle), the
designed inputs and per-element error bounds of tests/test_gpu_edm2_jvp_ops.py, and one MUTANT per plausible kernel error.
tests/test_edm2_jvp_ref.py shows on the CPU that each bound passes the fp32 oracle and separates every mutant by 5x or more on the GPU
test's own inputs.  CPU only, plain torch."""
import contextlib
import functools
import math

import torch
import torch.nn.functional as F
from torch.func import jvp

import edm2_ops_ref as R
import edm2_ref as D


def dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


# ---- cosine attention -----------------------------------------------------------------------------------------------------------------
# (B, T, heads): one query tile with two key tiles; several query tiles with batch and head offsets; a many-tile rescale
ATTN_JVP_SHAPES = [(1, 64, 1), (2, 128, 2), (1, 256, 3)]
ATTN_JVP_MUTANTS = ["u_term_dropped", "kd_term_dropped", "norm_projection_dropped", "alpha_dropped"]
ATTN_KEY_TILE = 32  # the kernel's key tile: what "alpha_dropped" depends on


def attn_jvp_inputs(B, T, heads, kind):
    """((q, k, v), (q_d, k_d, v_d)), each [B, heads, T, 64]: R.mp_attention_inputs with unit normal tangents."""
    seed = T + heads + len(kind)
    g = R.gen(seed + 1000)
    return R.mp_attention_inputs(B, T, heads, kind, seed), tuple(torch.randn(B, heads, T, 64, generator=g) for _ in range(3))


def attn_pack(q, k, v):
    """[B, heads, T, 64] x 3 -> the kernel's [B, T, heads * 192] (channel h * 192 + 3 c + j)."""
    B, heads, T, _ = q.shape
    return torch.stack([q, k, v], dim=-1).permute(0, 2, 1, 3, 4).reshape(B, T, heads * 192).contiguous()


def mp_attention_jvp_ref(prim, tang):
    """(out, out_d) of R.mp_attention_ref by torch.func.jvp, in the dtype of the inputs."""
    return jvp(lambda q, k, v: R.mp_attention_ref(q, k, v), tuple(prim), tuple(tang))


def mp_normalize_jvp(x, xd, mutant=None):
    """x^ = x / n, x^_d = x_d / n - x (x . x_d) / (8 |x| n^2), n = 1e-4 + |x| / 8; the tangent is x_d / 1e-4 where |x| = 0."""
    nx = torch.linalg.vector_norm(x, dim=-1, keepdim=True)
    n = 1e-4 + nx / 8
    dot = (x * xd).sum(-1, keepdim=True)
    proj = torch.where(nx > 0, dot / (8 * nx.clamp_min(1e-300 if x.dtype == torch.float64 else 1e-38) * n * n), torch.zeros_like(nx))
    if mutant == "norm_projection_dropped":
        proj = torch.zeros_like(proj)
    return x / n, xd / n - x * proj


def mp_normalize_jvp_mag(x, xd):
    """The sum of the magnitudes of the two terms of x^_d: what a rounding error of x^_d scales with (the terms may cancel)."""
    nx = torch.linalg.vector_norm(x, dim=-1, keepdim=True)
    n = 1e-4 + nx / 8
    dot = (x.abs() * xd.abs()).sum(-1, keepdim=True)
    proj = torch.where(nx > 0, dot / (8 * nx.clamp_min(1e-300) * n * n), torch.zeros_like(nx))
    return xd.abs() / n + x.abs() * proj


def mp_attention_jvp_formula(prim, tang, mutant=None):
    """(O, O_d) as the kernel computes them: s = q^ . k^ / 8, s_d = (q^_d . k^ + q^ . k^_d) / 8, p = exp(s - m), l = sum p,
    O = sum p v^ / l, O_d = sum p (s_d v^ + v^_d) / l - (sum p s_d / l) O.  alpha_dropped: the tangent sums of key tile j keep the
    running maximum of tiles 0 .. j instead of the final one."""
    (q, qd), (k, kd), (v, vd) = (mp_normalize_jvp(a, b, mutant) for a, b in zip(prim, tang))
    s = torch.einsum("bhqc,bhkc->bhqk", q, k) / 8
    sd = torch.einsum("bhqc,bhkc->bhqk", qd, k) / 8
    if mutant != "kd_term_dropped":
        sd = sd + torch.einsum("bhqc,bhkc->bhqk", q, kd) / 8
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    pt = p
    if mutant == "alpha_dropped":
        T = s.shape[-1]
        run = s.reshape(*s.shape[:-1], T // ATTN_KEY_TILE, ATTN_KEY_TILE).amax(-1).cummax(-1).values.repeat_interleave(ATTN_KEY_TILE, -1)
        pt = torch.exp(s - run)
    o = torch.einsum("bhqk,bhkc->bhqc", p, v) / l
    u = (pt * sd).sum(-1, keepdim=True) / l
    wz = (torch.einsum("bhqk,bhkc->bhqc", pt * sd, v) + torch.einsum("bhqk,bhkc->bhqc", pt, vd)) / l
    return o, wz if mutant == "u_term_dropped" else wz - u * o


def mp_attention_jvp_bound(prim, tang):
    """R.mp_attention_bound's form on the tangent's own magnitudes, per query: every term of O_d is a softmax average of s_d v^ or
    v^_d, so an error of relative size (4e-6 + 1e-6 max_k(|q^| . |k^|) / 8) - the primal's: the probabilities' error - scales with
    2 max_k(|q^_d| . |k^| + |q^| . |k^_d|) / 8 max|v^| + max|v^_d| (s_d enters twice: in w and in u O), the tangents of the rows
    taken as the sum of the magnitudes of their two terms."""
    q, k, v = (a.double() for a in prim)
    qd, kd, vd = (a.double() for a in tang)
    qn, kn, vn = R.mp_normalize(q), R.mp_normalize(k), R.mp_normalize(v)
    qa, ka, va = mp_normalize_jvp_mag(q, qd), mp_normalize_jvp_mag(k, kd), mp_normalize_jvp_mag(v, vd)
    mag = torch.einsum("bhqc,bhkc->bhqk", qn.abs(), kn.abs()).amax(-1, keepdim=True) / 8
    sda = (torch.einsum("bhqc,bhkc->bhqk", qa, kn.abs()) + torch.einsum("bhqc,bhkc->bhqk", qn.abs(), ka)).amax(-1, keepdim=True) / 8
    V, Vd = vn.abs().amax(dim=(2, 3), keepdim=True), va.amax(dim=(2, 3), keepdim=True)
    return (R.ATTN_C0 + R.ATTN_C1 * mag) * (2 * sda * V + Vd)


# ---- pixel norm -----------------------------------------------------------------------------------------------------------------------
PIXNORM_JVP_MUTANTS = {"projection_dropped": None, "down_x_only": 1}  # value: the `down` a mutant needs (None: any)
# the dot product x . x_d has mixed signs: a lane sums C / 64 <= 12 products, six shuffle levels follow, then about six roundings to
# the result: (12 + 6 + 6) 2^-24 < 2^-19 of the terms' magnitudes
PIXNORM_JVP_REL = 2.0 ** -19


def pixnorm_jvp_inputs(B, H, C, down):
    """(x, x_d) NCHW at the source resolution: R.pixnorm_inputs (one all-zero output pixel) with a unit normal tangent."""
    x = R.pixnorm_inputs(B, H, C, down)
    return x, torch.randn(x.shape, generator=R.gen(B + H + C + down + 1000))


def pixel_norm_jvp_ref(x, xd, down):
    return jvp(lambda a: R.pixel_norm_ref(a, down)[0], (x,), (xd,))[1]


def pixel_norm_jvp_formula(x, xd, down, mutant=None):
    """(out_d, its magnitude: the sum of the magnitudes of the two terms, window means of |.| under the 2x2 mean)."""
    rc = math.sqrt(x.shape[1])
    m = F.avg_pool2d(x, 2) if down else x
    md = xd[:, :, ::2, ::2] if down and mutant == "down_x_only" else F.avg_pool2d(xd, 2) if down else xd
    ma, mda = (F.avg_pool2d(x.abs(), 2), F.avg_pool2d(xd.abs(), 2)) if down else (x.abs(), xd.abs())
    nx = torch.linalg.vector_norm(m, dim=1, keepdim=True)
    n = 1e-4 + nx / rc
    safe = nx.clamp_min(1e-300 if x.dtype == torch.float64 else 1e-38)
    proj = torch.where(nx > 0, (m * md).sum(1, keepdim=True) / (rc * safe * n * n), torch.zeros_like(nx))
    proj_a = torch.where(nx > 0, (ma * mda).sum(1, keepdim=True) / (rc * safe * n * n), torch.zeros_like(nx))
    if mutant == "projection_dropped":
        proj = torch.zeros_like(proj)
    return md / n - m * proj, mda / n + ma * proj_a


# ---- SiLU operand ---------------------------------------------------------------------------------------------------------------------
# NHWC [B, hw, C1 + C2] over the virtual concat; ab as in R.CONV_EX_CASES: "ones" / "cat" one broadcast row (ab_stride 0) followed by
# B - 1 junk rows, "strided" rows of a [B, 200] matrix from element 72 with a_d rows of a second [B, 200] matrix (junk elsewhere).
SILU_CASES = {
    "bcast_ones": dict(C1=64, C2=0, hw=40, B=3, ab="ones"),
    "bcast_cat": dict(C1=96, C2=32, hw=24, B=3, ab="cat"),
    "strided": dict(C1=64, C2=0, hw=40, B=3, ab="strided"),
}
SILU_MUTANTS = {"ad_dropped": ["strided"], "row_image0": ["strided"], "bcast_row_per_image": ["bcast_ones", "bcast_cat"]}
# z = a x, the sigmoid, 1 - s (absolute 2^-24: |z| 2^-24 behind the product with z), the two products and their sum: about eight
# roundings of 2^-24 on the magnitude |a x_d| + |a_d x|, |silu'| <= 1.1
SILU_REL = 2.0 ** -20


def silu_inputs(name):
    """x, x_d [B, hw, C]; the ab buffer [rows, width, 2] with (ab_stride, first element); the a_d buffer [B, width] or None."""
    c = SILU_CASES[name]
    g = R.gen(sum(map(ord, name)) + 1000)
    B, C, hw = c["B"], c["C1"] + c["C2"], c["hw"]
    x, xd = 2.0 * torch.randn(B, hw, C, generator=g), torch.randn(B, hw, C, generator=g)
    if c["ab"] in ("ones", "cat"):
        ab = torch.stack([1 + 0.5 * torch.randn(B, C, generator=g), torch.zeros(B, C)], dim=-1)  # rows 1 ..: junk
        ab[0, :, 0] = 1.0
        if c["ab"] == "cat":
            ab[0, :c["C1"], 0], ab[0, c["C1"]:, 0] = 0.8164966, 1.4142135
        return x, xd, ab, 0, 0, None
    ab = torch.stack([1 + 0.5 * torch.randn(B, R.AB_STRIDE, generator=g), torch.zeros(B, R.AB_STRIDE)], dim=-1)
    ad = torch.randn(B, R.AB_STRIDE, generator=g)
    return x, xd, ab, R.AB_STRIDE, R.AB_OFF, ad


def silu_rows(name, mutant=None):
    """(a [B, 1, C], a_d [B, 1, C]): the rows the kernel reads (or, for a mutant, would read)."""
    c = SILU_CASES[name]
    B, C = c["B"], c["C1"] + c["C2"]
    _, _, ab, stride, off, ad = silu_inputs(name)
    step = C if mutant == "bcast_row_per_image" else 0 if mutant == "row_image0" else stride
    flat = ab.reshape(-1, 2)[:, 0]
    a = torch.stack([flat[off + b * step: off + b * step + C] for b in range(B)])
    if ad is None or mutant == "ad_dropped":
        a_d = torch.zeros_like(a)
    else:
        a_d = torch.stack([ad.reshape(-1)[off + b * step: off + b * step + C] for b in range(B)])
    return a[:, None], a_d[:, None]


def silu_operand_ref(name, dtype=torch.float64, mutant=None):
    """(the tangent of silu(a x) along (x_d, a_d) by torch.func.jvp, the bound's magnitude (1 + |a x|) (|a x_d| + |a_d x|))."""
    x, xd, _, _, _, _ = silu_inputs(name)
    a, a_d = silu_rows(name, mutant)
    x, xd, a, a_d = (t.to(dtype) for t in (x, xd, a, a_d))
    out = jvp(lambda u, w: F.silu(w * u), (x, a.expand_as(x).contiguous()), (xd, a_d.expand_as(x).contiguous()))[1]
    return out, (1 + (a * x).abs()) * ((a * xd).abs() + (a_d * x).abs())


def silu_operand_formula(name, dtype=torch.float32):
    x, xd, _, _, _, _ = silu_inputs(name)
    a, a_d = silu_rows(name)
    x, xd, a, a_d = (t.to(dtype) for t in (x, xd, a, a_d))
    return dsilu(a * x) * (a * xd + a_d * x)


# ---- blocks ---------------------------------------------------------------------------------------------------------------------------
def block_inputs(cfg, b, B, g):
    """x1, x2 (or None) and their tangents, unit normal, NCHW."""
    mk = lambda c: torch.randn(B, c, b.res_in, b.res_in, generator=g)  # noqa: E731
    x1, x1d = mk(b.cin - b.skip_c), mk(b.cin - b.skip_c)
    x2, x2d = (mk(b.skip_c), mk(b.skip_c)) if b.skip_c else (None, None)
    return x1, x1d, x2, x2d


def block_jvp_ref(sd64, b, cfg, x1, x1d, x2, x2d, emb, embd):
    """(out, out_d) of D.block (behind D.mp_cat for a decoder block with a skip) in fp64 by torch.func.jvp."""
    def f(a1, a2, e):
        return D.block(sd64, b, cfg, a1 if a2 is None else D.mp_cat(a1, a2, cfg.concat_balance), e)
    if x2 is None:
        return jvp(lambda a1, e: f(a1, None, e), (x1.double(), emb.double()), (x1d.double(), embd.double()))
    return jvp(f, (x1.double(), x2.double(), emb.double()), (x1d.double(), x2d.double(), embd.double()))


# One block with a low clip_act: the 8x8 attention block of SMALL_UNCOND (conv_skip, pixel norm, attention, the clamp behind the
# projection) at clip_act = 3, where a unit-variance activation clamps about 0.3 % of its elements.
LOW_CLIP, LOW_CLIP_BLOCK, LOW_CLIP_B = 3.0, 2, 2
LOW_CLIP_MARGIN = 100 * R.BLOCK_MAX_REL  # x max|pre-clamp|: 100 x the forward's per-element bound (bf16x3)


@functools.lru_cache(maxsize=None)
def low_clip_case():
    """The first seed at which no fp64 pre-clamp value of the block lies within LOW_CLIP_MARGIN max|pre| of +-clip: the mask the GPU
    takes from its own (rounded) output is then the oracle's.  Returns dict(seed, sd, cfg, b, inputs..., pre, pre_d)."""
    cfg = D.SMALL_UNCOND
    sd = D.random_state_dict(cfg, seed=97)
    sd64 = R.to64(sd)
    enc, dec, _, _, _ = D.layout(cfg)
    b = (enc + dec)[LOW_CLIP_BLOCK]
    assert b.attn and b.cin != b.cout
    free = D.EDM2Config(**{**cfg.__dict__, "clip_act": None})
    E = cfg.model_channels * max(cfg.channel_mult)
    for seed in range(2000):
        g = R.gen(5000 + seed)
        x1, x1d, x2, x2d = block_inputs(cfg, b, LOW_CLIP_B, g)
        emb, embd = torch.randn(LOW_CLIP_B, E, generator=g), torch.randn(LOW_CLIP_B, E, generator=g)
        with torch.no_grad():
            pre = D.block(sd64, b, free, x1.double(), emb.double())
        gap = ((pre.abs() - LOW_CLIP).abs().min() / pre.abs().max()).item()
        if gap > LOW_CLIP_MARGIN:
            pre, pre_d = block_jvp_ref(sd64, b, free, x1, x1d, x2, x2d, emb, embd)
            return dict(seed=seed, sd=sd, cfg=D.EDM2Config(**{**cfg.__dict__, "clip_act": LOW_CLIP}), b=b, x1=x1, x1d=x1d, emb=emb, embd=embd,
                        pre=pre, pre_d=pre_d, gap=gap)
    raise AssertionError("no seed keeps the pre-clamp values away from +-clip")


def clamp_jvp(pre, pre_d, clip, mutant=None):
    """The clamp's tangent: pre_d where |pre| < clip; mask_from_tangent: where |pre_d| < clip."""
    return pre_d * ((pre_d if mutant == "mask_from_tangent" else pre).abs() < clip)


# ---- the network ------------------------------------------------------------------------------------------------------------------------
# Structural mutants of the whole derivative (dropped terms), applied to the oracle through its own functions.  The last three need a
# tangent in t.
NET_MUTANTS = ["softmax_u_term_dropped", "kd_term_dropped", "norm_projection_dropped", "modulation_tangent_dropped", "c_out_d_F_dropped",
               "c_in_d_x_dropped"]
NET_MUTANTS_NEED_VT = {"modulation_tangent_dropped", "c_out_d_F_dropped", "c_in_d_x_dropped"}
TANGENTS = ["x", "t", "both"]


class _TorchProxy:
    """torch as tests/edm2_ref.py sees it, with the attention's softmax / logits losing one term of their tangent."""

    def __init__(self, mutant):
        self.mutant = mutant

    def __getattr__(self, name):
        return getattr(torch, name)

    def softmax(self, x, dim):
        if self.mutant != "softmax_u_term_dropped":
            return torch.softmax(x, dim)
        e = torch.exp(x - x.amax(dim, keepdim=True).detach())
        return e / e.sum(dim, keepdim=True).detach()

    def einsum(self, eq, a, b):
        if self.mutant == "kd_term_dropped" and eq == "bhcq,bhck->bhqk":
            b = b.detach()
        return torch.einsum(eq, a, b)


@contextlib.contextmanager
def mutated(mutant):
    """tests/edm2_ref.py with one term of its derivative dropped (detach() drops a tangent under torch.func.jvp)."""
    saved = (D.torch, D.pixel_norm, D.embedding)
    try:
        if mutant in ("softmax_u_term_dropped", "kd_term_dropped"):
            D.torch = _TorchProxy(mutant)
        elif mutant == "norm_projection_dropped":
            D.pixel_norm = lambda x, dim=1: x / (1e-4 + torch.linalg.vector_norm(x.detach(), dim=dim, keepdim=True) / math.sqrt(x.shape[dim]))
        elif mutant == "modulation_tangent_dropped":
            emb = saved[2]
            D.embedding = lambda *a, **k: emb(*a, **k).detach()
        yield
    finally:
        D.torch, D.pixel_norm, D.embedding = saved


def net_inputs(cfg, B, seed):
    """x_t, t (fp64), labels, v_x, v_t: x_t and v_x at the noise level's scale, v_t of the order of t (as sCM's dt is).  t runs from
    0.3 to 0.9, around sigma_data, where every t-derivative of the preconditioning (c_in, c_noise, c_skip, c_out) carries weight in
    every image: at t >> sigma_data c_out and c_skip saturate and a dropped c_out_d F term moves an image's derivative by 3 % only."""
    t = torch.exp(torch.linspace(math.log(0.3), math.log(0.9), B, dtype=torch.float64))
    g = R.gen(seed)
    scale = (cfg.sigma_data ** 2 + t ** 2).sqrt().float().reshape(-1, 1, 1, 1)
    x = torch.randn(B, cfg.img_channels, cfg.img_resolution, cfg.img_resolution, generator=g) * scale
    vx = torch.randn(x.shape, generator=g) * scale
    vt = (t * torch.tensor([1.0, -1.3] * B)[:B]).float()
    lab = F.one_hot(torch.arange(B) * 3 % cfg.label_dim, cfg.label_dim).float() if cfg.label_dim else None
    return x, t, lab, vx, vt


def precond_jvp(sd, cfg, x, t, lab, vx, vt, dtype=torch.float64, sigma_shift=0.0, drop_precond=None, mutant=None, trace=None):
    """(out, jvp) of D.precond_forward along (vx, vt) by torch.func.jvp; t stays fp64.  trace (a dict): the primal activations."""
    sdd = R.to64(sd) if dtype == torch.float64 else sd
    lab = None if lab is None else lab.to(dtype)

    def f(a, tt):
        if mutant == "c_in_d_x_dropped" and drop_precond not in ("input", "both"):
            # D.precond_forward restated with c_in's tangent dropped (the stem operand's c_in_d x term)
            sd2 = cfg.sigma_data ** 2
            c_in = (1 / (sd2 + tt ** 2).sqrt()).to(a.dtype).detach()
            c_noise = (tt.clamp(min=1e-6).log() / 4).to(a.dtype)
            F_x = D.unet(sdd, cfg, a * c_in[:, None, None, None], c_noise, lab)
            if drop_precond in ("output", "both"):
                return F_x
            ts = tt - sigma_shift
            c_skip, c_out = (sd2 / (ts ** 2 + sd2)).to(a.dtype), (ts * cfg.sigma_data / (ts ** 2 + sd2).sqrt()).to(a.dtype)
            return c_skip[:, None, None, None] * a + c_out[:, None, None, None] * F_x
        return D.precond_forward(sdd, cfg, a, tt, lab, sigma_shift=sigma_shift, drop_precond=drop_precond)

    with mutated(mutant):
        out, d = jvp(f, (x.to(dtype), t.double()), (vx.to(dtype), vt.double()))
    if trace is not None:
        with torch.no_grad():
            D.precond_forward(sdd, cfg, x.to(dtype), t.double(), lab, sigma_shift=sigma_shift, drop_precond=drop_precond, trace=trace)
    if mutant == "c_out_d_F_dropped" and drop_precond not in ("output", "both"):
        tr = {}
        with torch.no_grad():
            D.precond_forward(sdd, cfg, x.to(dtype), t.double(), lab, sigma_shift=sigma_shift, drop_precond=drop_precond, trace=tr)
        c_out_d = jvp(lambda tt: (tt - sigma_shift) * cfg.sigma_data / ((tt - sigma_shift) ** 2 + cfg.sigma_data ** 2).sqrt(), (t.double(),),
                      (vt.double(),))[1]
        d = d - c_out_d.to(dtype)[:, None, None, None] * tr["F"]
    return out, d


def tangent(kind, vx, vt):
    return (vx if kind != "t" else torch.zeros_like(vx)), (vt if kind != "x" else torch.zeros_like(vt))


def per_image(got, ref):
    """(worst per-image relative L2, max abs) of got against ref."""
    d = (got.double() - ref.double()).flatten(1)
    return (d.norm(dim=1) / ref.double().flatten(1).norm(dim=1).clamp_min(1e-300)).max().item(), d.abs().max().item()


def closest_image(mutant, ref):
    """The relative L2 distance of a mutated reference from the reference in the image where it is smallest: a threshold separates
    the mutant in every sample when this is 5x the threshold or more."""
    d = (mutant.double() - ref.double()).flatten(1)
    return (d.norm(dim=1) / ref.double().flatten(1).norm(dim=1).clamp_min(1e-300)).min().item()


# Thresholds of tests/test_gpu_edm2_jvp.py: worst per-image relative L2 and max |d| of the GPU's jvp against the fp64 oracle, about
# 1.5 x the values measured on an MI355X (see that test's docstring).
NET_JVP_TOL = {"bf16x3": dict(rel=2.7e-5, max_abs=1.0e-4), "bf16": dict(rel=1.3e-2, max_abs=6.2e-2)}
