"""fp64 mirror of the bidirectional video DiT's forward-mode derivative (fastgen_amd/csrc/wan_jvp.hip, engine_wan_jvp.inc `fg_wan_jvp`) -
TEST INFRASTRUCTURE ONLY.  One function per formula, a primal and a tangent side by side; tests/test_wan_jvp_ref.py pins every one
against `torch.func.jvp` of the corresponding piece of oracle/wan_ref.py (and the composition against tests/wan_full_ref.py's
`WanFullRef.forward`) and against a central difference.  `p` is the state dict without its `transformer.` prefix, in fp64.

`forward_rows` is the network on PER-FRAME embedder rows (ts, rs [B, F] in the embedder's units, as the C ABI's t_frames / r_frames) -
`WanFullRef.forward` with its one-t-per-sample preparation taken off - and `oracle_jvp` is `torch.func.jvp` over it: the whole-network
oracle of tests/test_gpu_wan_jvp.py.  `net_jvp` is the same tangent carried by hand through the mirror's functions.

The `drop_*` switches leave terms of the derivative out - the MUTANTS the GPU tests must tell the kernels from:
  (a) drop_delta   no softmax-derivative term: Od = P vd + (P o Sd) v
  (b) drop_pvd     P vd dropped
  (c) drop_gate    the gd o h terms of the gated residuals dropped
  (d) drop_mod     the n sd + bd terms of the LayerNorm-modulate dropped
  (e) drop_proj    the projection term of the RMSNorm's derivative dropped
  (f) flip_vr      v_r with the wrong sign                                   (input mutant: `mutant_rows`)
  (g) roll_vt      the neighbouring frame's vt / vr (rows rolled by one frame within a sample)  (input mutant: `mutant_rows`)"""
import ctypes
import math

import torch
import torch.nn.functional as F

from fastgen_amd import _lib
from oracle import wan_ref as R

MUTANTS = ("drop_delta", "drop_pvd", "drop_gate", "drop_mod", "drop_proj", "flip_vr", "roll_vt")


# ---- 1. time conditioning -------------------------------------------------------------------------------------------------------------
def fourier_jvp(t, td, dim):
    """[cos | sin](t f) and its tangent [-f sin | f cos] td; t, td [N]."""
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=t.dtype, device=t.device) / half)
    ang = t[:, None] * f[None, :]
    return torch.cat([ang.cos(), ang.sin()], -1), torch.cat([-f * ang.sin(), f * ang.cos()], -1) * td[:, None]


def silu_jvp(v, vd):
    sig = torch.sigmoid(v)
    return v * sig, sig * (1 + v * (1 - sig)) * vd


def embedder_jvp(p, cfg, t, td, prefix="condition_embedder."):
    """(temb, tembd, tproj, tprojd) of one time embedder on rows t [N]; the tangent of a linear has no bias."""
    W = lambda n: p[prefix + n + ".weight"]  # noqa: E731
    b = lambda n: p[prefix + n + ".bias"]  # noqa: E731
    f, fd = fourier_jvp(t, td, cfg.freq_dim)
    a, ad = silu_jvp(F.linear(f, W("time_embedder.linear_1"), b("time_embedder.linear_1")), F.linear(fd, W("time_embedder.linear_1")))
    e, ed = F.linear(a, W("time_embedder.linear_2"), b("time_embedder.linear_2")), F.linear(ad, W("time_embedder.linear_2"))
    s, sd = silu_jvp(e, ed)
    return e, ed, F.linear(s, W("time_proj"), b("time_proj")), F.linear(sd, W("time_proj"))


# ---- 2. LayerNorm-modulate ------------------------------------------------------------------------------------------------------------
def ln_modulate_jvp(x, xd, s, b, sd, bd, eps, drop_mod=False):
    """y = n (1 + s) + b with n = LN(x) over the last dim; s, b, sd, bd broadcast against x."""
    xc = x - x.mean(-1, keepdim=True)
    sig = (xc.pow(2).mean(-1, keepdim=True) + eps).sqrt()
    n = xc / sig
    nd = (xd - xd.mean(-1, keepdim=True) - n * (n * xd).mean(-1, keepdim=True)) / sig
    yd = nd * (1 + s)
    if not drop_mod:
        yd = yd + n * sd + bd
    return n * (1 + s) + b, yd


def per_frame_rows(m, L):
    """[B, F, D] modulation rows -> [B, L, D], every token its frame's row."""
    B, Fr, D = m.shape
    return m[:, :, None, :].expand(B, Fr, L // Fr, D).reshape(B, L, D)


# ---- 3. RMSNorm across heads (+ RoPE, linear) -----------------------------------------------------------------------------------------
def rms_jvp(x, xd, w, eps, drop_proj=False):
    rms = (x.pow(2).mean(-1, keepdim=True) + eps).sqrt()
    n = x / rms
    nd = xd if drop_proj else xd - n * (n * xd).mean(-1, keepdim=True)
    return n * w, nd / rms * w


def rope(x, cos, sin):
    """R.apply_rope without in-place writes (x [B, L, H, hd])."""
    x1, x2 = x[..., 0::2], x[..., 1::2]
    c, s = cos[None, :, None, 0::2], sin[None, :, None, 1::2]
    return torch.stack([x1 * c - x2 * s, x1 * s + x2 * c], -1).flatten(-2)


# ---- 4. attention ---------------------------------------------------------------------------------------------------------------------
def sdpa_plain(q, k, v):
    """R.sdpa without the fused kernel (forward-mode AD goes through it): [B, Lq, H, hd] x [B, Lk, H, hd] -> [B, Lq, H hd]."""
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(q.shape[-1])
    return torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), v).flatten(2)


def attention_jvp(q, k, v, qd, kd, vd, drop_delta=False, drop_pvd=False):
    """O = softmax(q k^T / sqrt(hd)) v and Od = (P o (Sd - delta)) v + P vd; kd / vd None: the keys carry no tangent.  [B, L, H, hd]
    operands, [B, Lq, H hd] results."""
    sc = 1.0 / math.sqrt(q.shape[-1])
    P = (torch.einsum("bqhd,bkhd->bhqk", q, k) * sc).softmax(-1)
    Sd = torch.einsum("bqhd,bkhd->bhqk", qd, k) * sc
    if kd is not None:
        Sd = Sd + torch.einsum("bqhd,bkhd->bhqk", q, kd) * sc
    Wm = P * Sd if drop_delta else P * (Sd - (P * Sd).sum(-1, keepdim=True))
    Od = torch.einsum("bhqk,bkhd->bqhd", Wm, v)
    if vd is not None and not drop_pvd:
        Od = Od + torch.einsum("bhqk,bkhd->bqhd", P, vd)
    return torch.einsum("bhqk,bkhd->bqhd", P, v).flatten(2), Od.flatten(2)


def attention_ref_distance(q, k, qd, kd, tile=32):
    """|c_i - delta_i| [B, Lq, H]: how far the kernel's per-query reference (the mean of Sd over the first key tile) stands from the
    softmax-weighted mean delta_i it replaces - the size at which W = P (Sd - c_i) is rounded to bf16."""
    sc = 1.0 / math.sqrt(q.shape[-1])
    P = (torch.einsum("bqhd,bkhd->bhqk", q, k) * sc).softmax(-1)
    Sd = torch.einsum("bqhd,bkhd->bhqk", qd, k) * sc
    if kd is not None:
        Sd = Sd + torch.einsum("bqhd,bkhd->bhqk", q, kd) * sc
    return (Sd[..., :tile].mean(-1) - (P * Sd).sum(-1)).abs().transpose(1, 2)


def attention_jvp_tiled(q, k, v, qd, kd, vd, c="mean", tile=32):
    """The kernel's algorithm restated tile by tile: 32-key tiles (a ragged last one), running maximum with the online rescale of l,
    O~, T and w, the per-query reference c_i taken at the first tile ("mean": the mean of Sd over it; a number or a [B, H, Lq] tensor:
    that reference), and at the end O = O~ / l, Od = T / l - (w / l) O."""
    sc = 1.0 / math.sqrt(q.shape[-1])
    B, Lq, H, hd = q.shape
    Lk = k.shape[1]
    m = torch.full((B, H, Lq), -math.inf, dtype=q.dtype)
    l, w = torch.zeros_like(m), torch.zeros_like(m)
    O, T = torch.zeros(B, H, Lq, hd, dtype=q.dtype), torch.zeros(B, H, Lq, hd, dtype=q.dtype)
    cref = None
    for j0 in range(0, Lk, tile):
        kt, vt = k[:, j0:j0 + tile], v[:, j0:j0 + tile]
        S = torch.einsum("bqhd,bkhd->bhqk", q, kt)
        Sd = torch.einsum("bqhd,bkhd->bhqk", qd, kt) * sc
        if kd is not None:
            Sd = Sd + torch.einsum("bqhd,bkhd->bhqk", q, kd[:, j0:j0 + tile]) * sc
        if cref is None:
            cref = Sd.mean(-1) if isinstance(c, str) else (c if torch.is_tensor(c) else torch.full_like(m, float(c)))
        mn = torch.maximum(m, S.amax(-1))
        alpha = torch.exp((m - mn) * sc)
        P = torch.exp((S - mn[..., None]) * sc)
        Wm = P * (Sd - cref[..., None])
        l, w = l * alpha + P.sum(-1), w * alpha + Wm.sum(-1)
        O = O * alpha[..., None] + torch.einsum("bhqk,bkhd->bhqd", P, vt)
        T = T * alpha[..., None] + torch.einsum("bhqk,bkhd->bhqd", Wm, vt)
        if vd is not None:
            T = T + torch.einsum("bhqk,bkhd->bhqd", P, vd[:, j0:j0 + tile])
        m = mn
    O = O / l[..., None]
    Od = T / l[..., None] - (w / l)[..., None] * O
    return O.transpose(1, 2).flatten(2), Od.transpose(1, 2).flatten(2)


# ---- 5. gated residual, 6. GELU -------------------------------------------------------------------------------------------------------
def gated_residual_jvp(x, xd, o, od, W, b, g=None, gd=None, drop_gate=False):
    """x' = x + g (W o + b);  xd' = xd + g (W od) + gd (W o + b).  g None: no gate (the cross-attention's residual)."""
    h = F.linear(o, W, b)
    if g is None:
        return x + h, xd + F.linear(od, W)
    yd = xd + g * F.linear(od, W)
    return x + g * h, yd if drop_gate else yd + gd * h


def gelu_jvp(h, hd):
    c0, c1 = math.sqrt(2.0 / math.pi), 0.044715
    sig = torch.sigmoid(2 * c0 * h * (1 + c1 * h * h))
    return h * sig, (sig + h * sig * (1 - sig) * 2 * c0 * (1 + 3 * c1 * h * h)) * hd


# ---- 8. output layer --------------------------------------------------------------------------------------------------------------------
def unpatchify(o, B, Fr, gh, gw):
    return o.view(B, Fr, gh, gw, 1, 2, 2, -1).permute(0, 7, 1, 4, 2, 5, 3, 6).reshape(B, -1, Fr, 2 * gh, 2 * gw)


def final_jvp(p, cfg, x, xd, so, sod, Fr, gh, gw, drop_mod=False):
    """so / sod [B, F, 2, D] = {shift, scale} rows and their tangents: out = b + W y, jvp = W yd, un-patchified."""
    B, L, _ = x.shape
    y, yd = ln_modulate_jvp(x, xd, per_frame_rows(so[:, :, 1], L), per_frame_rows(so[:, :, 0], L), per_frame_rows(sod[:, :, 1], L),
                            per_frame_rows(sod[:, :, 0], L), cfg.eps, drop_mod)
    return (unpatchify(F.linear(y, p["proj_out.weight"], p["proj_out.bias"]), B, Fr, gh, gw),
            unpatchify(F.linear(yd, p["proj_out.weight"]), B, Fr, gh, gw))


# ---- the network ------------------------------------------------------------------------------------------------------------------------
def _r_params(p):
    return {k.replace("r_embedder.", "condition_embedder."): v for k, v in p.items() if k.startswith("r_embedder.")}


def time_embedding(p, cfg, ts):
    """R.time_embedding on the device of ts (R.timesteps_proj builds its frequencies on the CPU)."""
    f = fourier_jvp(ts, ts, cfg.freq_dim)[0]
    return R._lin(p, F.silu(R._lin(p, f, "condition_embedder.time_embedder.linear_1")), "condition_embedder.time_embedder.linear_2")


def forward_rows(p, cfg, x, ts, rs, text, diff=True):
    """The raw network output on per-frame embedder rows ts, rs [B, F] (rs None: no r term), composed from oracle/wan_ref.py's pieces
    (attention through sdpa_plain).  Equal to WanFullRef.forward when a sample's rows are all 1000 t / 1000 r."""
    B, C, Fr, H, W = x.shape
    gh, gw = H // 2, W // 2
    cos, sin = (v.to(x.device) for v in R.rope_for_chunk(cfg, Fr, gh, gw, 0, x.dtype))
    hs = R.patch_embed(p, x)
    temb = time_embedding(p, cfg, ts.reshape(-1))
    tproj = R.time_projection(p, temb)
    if rs is not None:
        pr = _r_params(p)
        remb = time_embedding(pr, cfg, (ts - rs if diff else rs).reshape(-1))
        tproj, temb = tproj + R.time_projection(pr, remb), temb + remb
    ctx = R.text_embedding(p, text)
    for i in range(cfg.num_layers):
        b = f"blocks.{i}."
        mod = R.modulation(p, i, tproj, B, Fr)
        L = hs.shape[1]
        y = R.per_frame(R.layer_norm(hs, cfg.eps), mod[:, :, 1], mod[:, :, 0])
        q = R.rms_norm(R._lin(p, y, b + "attn1.to_q"), p[b + "attn1.norm_q.weight"], cfg.eps).view(B, L, cfg.num_heads, -1)
        k = R.rms_norm(R._lin(p, y, b + "attn1.to_k"), p[b + "attn1.norm_k.weight"], cfg.eps).view(B, L, cfg.num_heads, -1)
        v = R._lin(p, y, b + "attn1.to_v").view(B, L, cfg.num_heads, -1)
        hs = R.self_attn_out(p, i, hs, sdpa_plain(rope(q, cos, sin), rope(k, cos, sin), v), mod)
        k2, v2 = R.cross_kv(p, cfg, i, ctx)
        y = R.layer_norm(hs, cfg.eps, p[b + "norm2.weight"], p[b + "norm2.bias"])
        q2 = R.rms_norm(R._lin(p, y, b + "attn2.to_q"), p[b + "attn2.norm_q.weight"], cfg.eps).view(B, L, cfg.num_heads, -1)
        hs = hs + R._lin(p, sdpa_plain(q2, k2, v2), b + "attn2.to_out.0")
        hs = R.ffn(p, cfg, i, hs, mod)
    return R.final_layer(p, cfg, hs, temb, Fr, gh, gw)


def oracle_jvp(p, cfg, x, ts, rs, text, vx, vts, vrs, diff=True):
    """(out, jvp) = torch.func.jvp over forward_rows in (x, ts, rs)."""
    if rs is None:
        return torch.func.jvp(lambda a, b: forward_rows(p, cfg, a, b, None, text, diff), (x, ts), (vx, vts))
    return torch.func.jvp(lambda a, b, c: forward_rows(p, cfg, a, b, c, text, diff), (x, ts, rs), (vx, vts, vrs))


def mutant_rows(name, vts, vrs):
    """The input mutants (f), (g): the tangent rows a wrong engine would have used."""
    if name == "flip_vr":
        return vts, -vrs
    if name == "roll_vt":
        return vts.roll(1, dims=1), (vrs.roll(1, dims=1) if vrs is not None else None)
    raise ValueError(name)


def net_jvp(p, cfg, x, ts, rs, text, vx, vts, vrs, diff=True, drop_delta=False, drop_pvd=False, drop_gate=False, drop_mod=False,
            drop_proj=False):
    """fg_wan_jvp's schedule in fp64: (out, jvp), the tangent carried by hand through the functions above."""
    B, C, Fr, H, W = x.shape
    gh, gw, nh = H // 2, W // 2, cfg.num_heads
    cos, sin = (v.to(x.device) for v in R.rope_for_chunk(cfg, Fr, gh, gw, 0, x.dtype))
    temb, tembd, tproj, tprojd = embedder_jvp(p, cfg, ts.reshape(-1), vts.reshape(-1))
    if rs is not None:
        rr, rrd = ((ts - rs), (vts - vrs)) if diff else (rs, vrs)
        e, ed, pj, pjd = embedder_jvp(_r_params(p), cfg, rr.reshape(-1), rrd.reshape(-1))
        temb, tembd, tproj, tprojd = temb + e, tembd + ed, tproj + pj, tprojd + pjd
    hs = R.patch_embed(p, x)
    hd = F.conv3d(vx, p["patch_embedding.weight"], None, stride=(1, 2, 2)).flatten(2).transpose(1, 2)
    L, D = hs.shape[1], hs.shape[2]
    ctx = R.text_embedding(p, text)
    modd = tprojd.view(B, Fr, 6, D)  # (the tangent of table + tproj is tproj's)
    row = lambda m, j: per_frame_rows(m[:, :, j], L)  # noqa: E731
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    for i in range(cfg.num_layers):
        b = f"blocks.{i}."
        lin = lambda a, n, bias=True: F.linear(a, p[b + n + ".weight"], p[b + n + ".bias"] if bias else None)  # noqa: E731
        mod = R.modulation(p, i, tproj, B, Fr)
        y, yd = ln_modulate_jvp(hs, hd, row(mod, 1), row(mod, 0), row(modd, 1), row(modd, 0), cfg.eps, drop_mod)
        q, qd = rms_jvp(lin(y, "attn1.to_q"), lin(yd, "attn1.to_q", False), p[b + "attn1.norm_q.weight"], cfg.eps, drop_proj)
        k, kd = rms_jvp(lin(y, "attn1.to_k"), lin(yd, "attn1.to_k", False), p[b + "attn1.norm_k.weight"], cfg.eps, drop_proj)
        v, vd = lin(y, "attn1.to_v"), lin(yd, "attn1.to_v", False)
        hv = lambda a: a.view(B, -1, nh, cfg.head_dim)  # noqa: E731
        o, od = attention_jvp(rope(hv(q), cos, sin), rope(hv(k), cos, sin), hv(v), rope(hv(qd), cos, sin), rope(hv(kd), cos, sin), hv(vd),
                              drop_delta, drop_pvd)
        hs, hd = gated_residual_jvp(hs, hd, o, od, p[b + "attn1.to_out.0.weight"], p[b + "attn1.to_out.0.bias"], row(mod, 2), row(modd, 2),
                                    drop_gate)
        k2, v2 = R.cross_kv(p, cfg, i, ctx)
        y, yd = ln_modulate_jvp(hs, hd, p[b + "norm2.weight"] - 1, p[b + "norm2.bias"], zero, zero, cfg.eps)
        q2, q2d = rms_jvp(lin(y, "attn2.to_q"), lin(yd, "attn2.to_q", False), p[b + "attn2.norm_q.weight"], cfg.eps, drop_proj)
        o, od = attention_jvp(hv(q2), k2, v2, hv(q2d), None, None, drop_delta, drop_pvd)
        hs, hd = gated_residual_jvp(hs, hd, o, od, p[b + "attn2.to_out.0.weight"], p[b + "attn2.to_out.0.bias"])
        y, yd = ln_modulate_jvp(hs, hd, row(mod, 4), row(mod, 3), row(modd, 4), row(modd, 3), cfg.eps, drop_mod)
        a, ad = gelu_jvp(lin(y, "ffn.net.0.proj"), lin(yd, "ffn.net.0.proj", False))
        hs, hd = gated_residual_jvp(hs, hd, a, ad, p[b + "ffn.net.2.weight"], p[b + "ffn.net.2.bias"], row(mod, 5), row(modd, 5), drop_gate)
    so = p["scale_shift_table"].view(1, 1, 2, D) + temb.view(B, Fr, 1, D)
    sod = tembd.view(B, Fr, 1, D).expand(B, Fr, 2, D)
    return final_jvp(p, cfg, hs, hd, so, sod, Fr, gh, gw, drop_mod)


def mutant_jvp(name, p, cfg, x, ts, rs, text, vx, vts, vrs, diff=True):
    """The tangent under mutant `name` (MUTANTS)."""
    if name in ("flip_vr", "roll_vt"):
        a, b = mutant_rows(name, vts, vrs)
        return net_jvp(p, cfg, x, ts, rs, text, vx, a, b, diff)[1]
    return net_jvp(p, cfg, x, ts, rs, text, vx, vts, vrs, diff, **{name: True})[1]


# ---- shared inputs of the CPU and GPU tests ---------------------------------------------------------------------------------------------
def params64(sd, device="cpu"):
    return {k[len("transformer."):]: v.double().to(device) for k, v in sd.items()}


def frame_rows(B, Fr, seed, with_r=True):
    """ts, rs, vts, vrs [B, F] fp32-exact fp64 rows: every frame its own t and r (2 B F distinct points of [50, 950], t - r > 0, as
    tests/test_gpu_wan_blocks.py::_inputs), its own vt around 1000 (the derivative of the x1000 timestep scale on v_t = 1, spread
    +-30 % so that a neighbouring frame's row is a different number) and its own vr of the same size."""
    g = torch.Generator().manual_seed(seed)
    n = B * Fr
    v = (0.05 + 0.9 * (torch.randperm(2 * n, generator=g).double() + 0.5) / (2 * n)).view(n, 2)
    ts, rs = (1000.0 * v.amax(1)).float().double().view(B, Fr), (1000.0 * v.amin(1)).float().double().view(B, Fr)
    vts = (1000.0 * (0.7 + 0.6 * torch.rand(B, Fr, generator=g))).float().double()
    vrs = (1000.0 * (0.7 + 0.6 * torch.rand(B, Fr, generator=g)) * (torch.randint(0, 2, (B, Fr), generator=g) * 2 - 1)).float().double()
    return ts, (rs if with_r else None), vts, (vrs if with_r else None)


def rel_l2(a, b, dims=None):
    """Relative L2 of a against b, per sample (dim 0 kept) unless dims is given."""
    dims = tuple(range(1, a.ndim)) if dims is None else dims
    return (a - b).pow(2).sum(dims).sqrt() / b.pow(2).sum(dims).sqrt()


# ---- the cases of tests/test_gpu_wan_jvp.py (2-layer networks, text 37 tokens of 64 dims, Q_GAIN on norm_q as the per-block pins) --------
MUTANT_FACTOR = 5.0  # (tests/test_gpu_wan_blocks.py's; asserted equal there)
Q_GAIN = 3.0
NET_CASES = {
    "F105": dict(B=1, frames=7, lat=(10, 6), heads=2, ffn=512, r="diff"),          # 7 frames x 15 tokens
    "F105-nor": dict(B=1, frames=7, lat=(10, 6), heads=2, ffn=512, r=""),          # a handle without the r_embedder
    "F480-diff": dict(B=2, frames=5, lat=(16, 24), heads=2, ffn=512, r="diff"),    # 5 frames x 96 tokens
    "F480-abs": dict(B=2, frames=5, lat=(16, 24), heads=2, ffn=512, r="abs"),
    "F1152": dict(B=2, frames=12, lat=(16, 24), heads=2, ffn=512, r="diff", device=True),  # > 1024 keys; the oracle runs on the device
    "F105-D1536": dict(B=1, frames=7, lat=(10, 6), heads=12, ffn=8960, r="diff"),
}


def net_case_weights(name):
    c = NET_CASES[name]
    import wan_full_ref

    gh, gw = c["lat"][0] // 2, c["lat"][1] // 2
    cfg = R.WanConfig(num_heads=c["heads"], head_dim=128, in_channels=16, out_channels=16, text_dim=64, ffn_dim=c["ffn"], num_layers=2,
                      rope_max_seq_len=max(c["frames"], gh, gw), chunk_size=1, total_num_frames=1)
    seed = 5000 + 7 * c["heads"] + c["B"] + c["frames"]
    sd = wan_full_ref.random_state_dict(cfg, seed=seed, r_timestep=bool(c["r"]))
    for k in sd:
        if k.endswith("attn1.norm_q.weight"):
            sd[k] = sd[k] * Q_GAIN
    return cfg, sd, seed


def net_case(name, device="cpu", batch=None):
    """(cfg, p, x, ts, rs, vts, vrs, text, vx) in fp64 on `device`; x, vx, text are fp32-exact.  batch: another batch size on the same
    weights (sample b's inputs do not depend on it)."""
    c = NET_CASES[name]
    cfg, sd, seed = net_case_weights(name)
    B = batch or c["B"]
    shp = (cfg.in_channels, c["frames"]) + tuple(c["lat"])
    gen = lambda b, k, *s: torch.randn(*s, generator=torch.Generator().manual_seed(100 * seed + 10 * b + k)).double()  # noqa: E731
    x = torch.stack([gen(b, 0, *shp) for b in range(B)])
    vx = torch.stack([gen(b, 1, *shp) for b in range(B)])
    text = torch.stack([gen(b, 2, 37, cfg.text_dim) for b in range(B)])
    rows = [frame_rows(1, c["frames"], 100 * seed + 10 * b + 3, bool(c["r"])) for b in range(B)]
    ts, rs, vts, vrs = (torch.cat([r[i] for r in rows]) if rows[0][i] is not None else None for i in range(4))
    to = lambda v: None if v is None else v.to(device)  # noqa: E731
    return (cfg, params64(sd, device)) + tuple(to(v) for v in (x, ts, rs, vts, vrs, text, vx))


def make_handle(dtype=None, kind="ex", r=1):
    """An unpacked fg_wan handle through the C ABI: kind "ex" (plain text-to-video), "i2v" or "vace"; the caller destroys it."""
    L = _lib.lib()
    cfg = _lib.fg_wan_config()
    cfg.compute_dtype = _lib.DTYPE_NAMES[dtype or "bf16"]
    cfg.num_heads, cfg.head_dim, cfg.in_channels, cfg.out_channels = 2, 128, 16, 16
    cfg.text_dim, cfg.freq_dim, cfg.ffn_dim, cfg.num_layers = 64, 256, 512, 2
    cfg.rope_max_seq_len, cfg.chunk_size, cfg.total_num_frames, cfg.eps = 16, 1, 1, 1e-6
    ext = _lib.fg_wan_ext_config()
    ext.r_timestep, ext.time_cond_diff = r, 1
    h = ctypes.c_void_p()
    if kind == "i2v":
        cfg.in_channels = 36
        i2v = _lib.fg_wan_i2v_config()
        i2v.latent_channels, i2v.mask_channels, i2v.image_dim = 16, 4, 0
        _lib.check(L.fg_wan_create_i2v(ctypes.byref(cfg), ctypes.byref(ext), ctypes.byref(i2v), ctypes.byref(h)))
    elif kind == "vace":
        vace = _lib.fg_wan_vace_config()
        vace.vace_in_channels, vace.num_vace_layers = 96, 1
        vace.vace_layers[0] = 0
        _lib.check(L.fg_wan_create_vace(ctypes.byref(cfg), ctypes.byref(ext), ctypes.byref(vace), ctypes.byref(h)))
    else:
        _lib.check(L.fg_wan_create_ex(ctypes.byref(cfg), ctypes.byref(ext), ctypes.byref(h)))
    return h


# ---- the cases of the attention op in tests/test_gpu_wan_jvp_ops.py ----------------------------------------------------------------------
ATT_CASES = {
    "ragged": dict(B=2, H=2, Lq=105, Lk=105),               # one ragged query tile, waves without rows, a 9-key last tile
    "many": dict(B=1, H=3, Lq=555, Lk=555),                 # five query tiles, 18 key tiles of rescaling
    "long": dict(B=1, H=2, Lq=1152, Lk=1152),               # more than 1024 keys
    "cross": dict(B=2, H=2, Lq=105, Lk=37, cross=True),     # interleaved k | v rows, null kd and vd
    "vd-only": dict(B=2, H=2, Lq=105, Lk=105, zero=("qd", "kd")),   # Od = P vd
    "no-vd": dict(B=2, H=2, Lq=105, Lk=105, zero=("vd",)),
    "shift": dict(B=2, H=2, Lq=105, Lk=105, shift=True),    # kd plus one row common to all keys
}
ATT_MUTANT_SKIP = {"drop_delta": ("vd-only",), "drop_pvd": ("no-vd",)}  # (where the mutant is the same function)


def bf16_exact(v):
    return v.float().bfloat16().double()


def att_case(name, device="cpu"):
    """q, k, v, qd, kd, vd [B, L, H, 128] fp64 with bf16-exact values (the kernel reads the same numbers); kd, vd None for "cross"."""
    c = ATT_CASES[name]
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    g = torch.Generator().manual_seed(7000 + Lq + 3 * Lk + H)
    mk = lambda L, s=1.0: bf16_exact(s * torch.randn(B, L, H, 128, generator=g)).to(device)  # noqa: E731
    q, k, v, qd, kd, vd = mk(Lq, Q_GAIN), mk(Lk), mk(Lk), mk(Lq, Q_GAIN), mk(Lk), mk(Lk)
    for z in c.get("zero", ()):
        if z == "qd":
            qd = torch.zeros_like(qd)
        elif z == "kd":
            kd = torch.zeros_like(kd)
        else:
            vd = torch.zeros_like(vd)
    if c.get("shift"):
        kd = bf16_exact(kd + COMMON_SHIFT * torch.randn(B, 1, H, 128, generator=g).double().to(device))
    if c.get("cross"):
        kd = vd = None
    return q, k, v, qd, kd, vd


# The size of the key-common row of the "shift" case relative to the rest of kd: what tests/test_wan_jvp_ref.py::test_common_shift_ratio
# measures in fp64 in the whole-network time direction (0, 1, 0) of case F105 (block 0 / block 1: see there), rounded up.
COMMON_SHIFT = 2.0

# ---- bounds: (relative L2, max |err| / max |ref|) per granule = twice the worst measured on an MI355X over each matrix -----------------
# Network (tests/test_gpu_wan_jvp.py), per sample, over J.NET_CASES x the three directions: worst 9.05e-3 / 1.18e-2, both at F105 in
# the direction x (the time directions sit at 5.5e-3 ... 7.0e-3, F1152 at 8.1e-3 / 1.03e-2 in x); the module-level call 5.96e-3 / 6.9e-3.
# `out` against fp64: 4.82e-3 at worst (F1152; bound 2e-2), against fg_wan_forward_full 3.65e-3 (F1152).
# Mutants, closest sample over the six cases as a multiple of NET_TOL[0]: (a) drop_delta 12 (F480-diff), (c) drop_gate 24 (F480-abs),
# (d) drop_mod 103 (F105), (f) flip_vr 58 (F480-diff), (g) roll_vt 15 (F105-nor).  Two do not separate by MUTANT_FACTOR under bf16 and
# are left to the per-op file: (b) drop_pvd 5.02 (F480-diff: 9.1e-2 from the GPU; v's tangent is a small part of the attention output's
# in the time direction) and (e) drop_proj 1.2 (F105-D1536: 2.2e-2; the projection term is 1 / sqrt(D) of the RMSNorm's tangent).
NET_TOL = (1.81e-2, 2.36e-2)
NET_WEAK_MUTANTS = ("drop_pvd", "drop_proj")
# Attention op (tests/test_gpu_wan_jvp_ops.py), Od over the un-shifted cases of J.ATT_CASES; the "shift" case must hold the same bounds
# (it gave 3.92e-3 / 8.81e-3 per (sample, head) and 2.96e-2 / 3.53e-2 per query):
#   per (sample, head): 4.04e-3 (no-vd) / 7.16e-3 (ragged)
#   per (sample, query, head), cases with a vd term (ragged, many, long, vd-only, shift): 2.33e-2 / 2.82e-2 (ragged)
#   (the cases without a P vd term, cross and no-vd, have no relative per-query bound: a row of Od is then (P o (Sd - delta)) v alone,
#   as small as that query's softmax is peaked, while W is rounded to bf16 at c_i, not at delta_i - 1.9e-1 / 1.7e-1 relative in the
#   worst row of cross; the scaled bound below is what holds their rows, and per (sample, head) they sit where the others sit)
#   per (sample, query, head), scaled ("od/row-scaled"): |err row| / (|Od row| + |c_i - delta_i| rms_j |v_j|), the row's own size plus
#   the size W is rounded at (attention_ref_distance) - 3.45e-3 (many), and 2.5e-3 ... 3.4e-3 in EVERY case, cross, no-vd and shift
#   (3.18e-3) included.
# The kernel's primal O: 2.81e-3 / 4.85e-3 per query, 1.81e-3 / 3.03e-3 per (sample, head) - inside the existing attn1 bounds.
# Mutants, closest sample as a multiple of ATT_TOL["od"][0]: drop_delta 63 (long), drop_pvd 43 (long).
ATT_TOL = {"od": (8.1e-3, 1.43e-2), "od/row": (4.66e-2, 5.64e-2), "od/row-scaled": 6.9e-3}
