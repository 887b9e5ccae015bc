"""CPU checks of tests/edm_ops_ref.py, the fp64 references the GPU tests of the SongUNet inference kernels compare against
(test_gpu_edm_ops.py): (1) an fp32 / bf16 emulation of each kernel's arithmetic, written in torch from the kernels' header comments,
stays inside the bound on EVERY element of every designed input - the bounds are not too tight for correct arithmetic; (2) every named
mutation of a reference (edm_ops_ref.MUTANTS: what a subtly wrong kernel would compute) lies at least 5 bounds away on at least one
element of a named case, in each storage type it applies to - the inputs can see each error; (3) the bounds are small against the
values: median(bound / max|value| of the image) <= 2^-12 in the fp32 and bf16x3 modes, 2^-6 in bf16 storage (the mean-offset cases,
whose bound is meant to grow, excluded); (4) the fg_op_edm_* entry points refuse, before any launch and without a GPU, what their
launchers cannot serve, and fg_op_edm_conv_plan names the kernel and slot count the dispatch will take.

The emulation is independent of the reference in its ARITHMETIC only.  It shares the reference's index conventions - R.concat,
R.qkv_weight (the q | k | v de-interleave), R.slot_map (which pixels a statistics slot holds) and R.gn_geometry - so an error in one of
those passes here unseen; the run against the kernels (test_gpu_edm_ops.py) is what pins them."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from fastgen_amd import _lib

import edm_ops_ref as R

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LIMIT = {0: 2.0 ** -12, 1: 2.0 ** -6, 2: 2.0 ** -12}
MODE_IDS = R.MODE_NAME.get


# ---- the emulations: fp32 tensors, the roundings the headers name ------------------------------------------------------------------------

def fma32(a, x, b):
    return (a.to(F64) * x.to(F64) + b.to(F64)).to(F32)  # the product is exact in fp64: one rounding, as v_fma_f32


def rnd_store(v, mode):
    return v.to(BF16).to(F32) if mode == 1 else v


def split(v):
    hi = v.to(BF16).to(F32)
    return hi, (v - hi).to(BF16).to(F32)


def mm(a, b, mode, op=torch.matmul):
    """A product sum on the matrix cores: fp32 (mode 0), bf16 operands (mode 1), three bf16 partial products (mode 2)."""
    if mode == 1:
        return op(a.to(BF16).to(F32), b.to(BF16).to(F32))
    if mode == 2:
        (ah, al), (bh, bl) = split(a), split(b)
        return op(al, bh) + op(ah, bl) + op(ah, bh)
    return op(a, b)


def emu_pro(x, ab, pro):
    if pro == R.PRO_NONE:
        return x
    y = fma32(ab[:, None, None, :, 0].to(F32), x, ab[:, None, None, :, 1].to(F32))
    return y if pro == R.PRO_GN else y * torch.sigmoid(y)


def emu_resample(t, res):
    if res == R.RES_DOWN:
        return 0.25 * (((t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + t[:, 1::2, 0::2]) + t[:, 1::2, 1::2])
    if res in (R.RES_UP, R.RES_SUBPIX):
        return t.repeat_interleave(2, 1).repeat_interleave(2, 2)
    return t


def emu_conv_core(op_nhwc, w, mode):
    p = w.shape[-1] // 2
    conv = lambda a, b: F.conv2d(a, b, padding=p)
    return mm(op_nhwc.permute(0, 3, 1, 2), w.to(F32), mode, conv).permute(0, 2, 3, 1)


def emu_conv(d, mode):
    w = R.qkv_weight(d["w"]) if d.get("qkv_perm") else d["w"]
    acc = emu_conv_core(emu_resample(emu_pro(R.concat(d).to(F32), d.get("ab"), d["pro"]), d["res"]), w, mode)
    B, H, W, Cout = acc.shape
    v = acc + d["bias"].to(F32)
    if d["outmode"] != R.OUT_NHWC:
        planes = v.reshape(B, H * W, Cout // 256, 256).unbind(2)
        names = ("q", "k", "vt") if d["outmode"] == R.OUT_QKV else ("q", "vt")
        return {n: rnd_store(p.transpose(1, 2) if n == "vt" else p, mode).to(F64) for n, p in zip(names, planes)}
    if d.get("temb") is not None:
        v = v + d["temb"].to(F32)[:, None, None, :]
    if d.get("resid") is not None:
        r = d["resid"].to(F32)
        v = v + (r.repeat_interleave(2, 1).repeat_interleave(2, 2) if d.get("rshift") else r)
    return {"out": rnd_store(v * torch.tensor(d.get("scale", 1.0), dtype=F32), mode).to(F64)}


def emu_slot_stats(v, layout):
    B, H, _, C = v.shape
    ids, S = R.slot_map(layout, H)
    onehot = F.one_hot(ids.reshape(-1), S).to(F32)
    q = v.to(F32).reshape(B, H * H, C // 4, 4)
    return torch.stack([torch.einsum("ps,bpq->bsq", onehot, q.sum(-1)), torch.einsum("ps,bpq->bsq", onehot, (q * q).sum(-1))], -1).to(F64)


def emu_gn_finalize(st1, st2, gamma, beta, eps, hw):
    quads = torch.cat([s.sum(1) for s in (st1, st2) if s is not None], 1)
    B, Q, _ = quads.shape
    G, cpg = R.gn_geometry(4 * Q)
    S = quads.reshape(B, G, cpg // 4, 2).sum(2)
    mean = S[..., 0] / (cpg * hw)
    var = (S[..., 1] / (cpg * hw) - mean * mean).clamp_min(0.0)
    m, rstd = mean.to(F32), ((var + eps) ** -0.5).to(F32)
    a = rstd.repeat_interleave(cpg, 1) * gamma.to(F32)
    b = fma32(-a, m.repeat_interleave(cpg, 1), beta.to(F32))
    return torch.stack([a, b], -1).to(F64), torch.stack([m, rstd], -1).to(F64)


def emu_attention(q, k, vt, mode):
    s = mm(q.to(F32), k.to(F32).transpose(-1, -2), mode)
    z = (s - s.amax(-1, keepdim=True)) * 0.0625
    e = torch.exp(z)
    P = e / e.sum(-1, keepdim=True)
    return rnd_store(mm(P, vt.to(F32).transpose(-1, -2), mode), mode).to(F64)


def emu_attention_merged(qm, x_mid, ab, vmt, bp, scale):
    xn = fma32(ab[:, None, :, 0].to(F32), x_mid.to(F32), ab[:, None, :, 1].to(F32))
    s = mm(qm.to(F32), xn.transpose(-1, -2), 2)
    e = torch.exp((s - s.amax(-1, keepdim=True)) * 0.0625)
    o = mm(e / e.sum(-1, keepdim=True), vmt.to(F32).transpose(-1, -2), 2)
    return ((o + bp.to(F32) + x_mid.to(F32)) * torch.tensor(scale, dtype=F32)).to(F64)


def emu_stem(x, c_in, w, bias, mode, mfma):
    v = (c_in.to(F32)[:, None, None, None] * x.to(F32)).permute(0, 2, 3, 1)
    return rnd_store(emu_conv_core(v, w, 1 if (mfma and mode == 1) else 0) + bias.to(F32), mode).to(F64)


def emu_aux(x, ab, w, bias, x_t, coef, mode, mfma):
    B = x.shape[0]
    Fv = (emu_conv_core(emu_pro(x.to(F32), ab, R.PRO_GN_SILU), w, mode if mfma else 0) + bias.to(F32)).permute(0, 3, 1, 2)
    c = coef.to(F32)
    return (c[2 * B:3 * B, None, None, None] * x_t.to(F32) + c[3 * B:4 * B, None, None, None] * Fv).to(F64)


# ---- helpers -------------------------------------------------------------------------------------------------------------------------------

def worst(got, ref, bound):
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return torch.nan_to_num(r, nan=float("inf")).max().item()


def assert_bound_small(tag, v, b, mode):
    assert torch.isfinite(b).all() and (b >= 0).all(), tag
    med = (b / v.abs().max().clamp_min(1e-300)).median().item()
    assert med <= LIMIT[mode], (tag, med / LIMIT[mode])


@functools.lru_cache(maxsize=None)
def conv_ref(name, mode):
    d = R.conv_inputs(name, mode)
    return d, R.conv(d, mode)


CONV_PARAMS = [(n, m) for n in R.CONV_CASES for m in R.conv_modes(n)]
CONV_IDS = [f"{n}-{R.MODE_NAME[m]}" for n, m in CONV_PARAMS]


def head_inputs(mode, B, res=32, C=128, cout=3):
    g = torch.Generator().manual_seed(7000 + B + mode)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    ts = [0.002, 80.0, 1.0][:B]
    return dict(x_t=R.f32r(rn(B, cout, res, res) * torch.tensor(ts, dtype=F64)[:, None, None, None]), coef=R.edm_coef(ts),
                w_stem=R.f32r(rn(128, cout, 3, 3) / 27 ** 0.5), b_stem=R.f32r(rn(128)),
                x=R.to_storage(R.bordered(rn(B, res, res, C)), mode), ab=R.design_ab(B, C, g),
                w_aux=R.f32r(rn(cout, C, 3, 3) / (9 * C) ** 0.5), b_aux=R.f32r(rn(cout)))


# ---- (1) the emulation passes every bound, (3) the bounds are small ------------------------------------------------------------------------

@pytest.mark.parametrize("name,mode", CONV_PARAMS, ids=CONV_IDS)
def test_conv_emulation_and_bound(name, mode):
    d, ref = conv_ref(name, mode)
    got = emu_conv(d, mode)
    for key, (v, b) in ref.items():
        assert worst(got[key], v, b) <= 1.0, (name, key, worst(got[key], v, b))
        assert_bound_small(f"{name} {key}", v, b, mode)
    if d["outmode"] == R.OUT_NHWC:  # the statistics of the tensor as stored, in every slot layout a kernel may write
        for layout in ("tile", "x3") + (("x3sub",) if d["res"] == R.RES_SUBPIX else ()):
            sv, sb = R.slot_stats(got["out"], layout)
            assert worst(emu_slot_stats(got["out"], layout), sv, sb) <= 1.0, (name, layout)
            assert_bound_small(f"{name} stats {layout}", sv[..., 0], sb[..., 0], 0)


@pytest.mark.parametrize("mode", R.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("offset", R.GN_OFFSETS)
def test_mean_offset_chain_emulation(mode, offset):
    """conv -> slots -> gn_finalize at a per-group mean / std of `offset`: the emulated chain's normalised value against the GroupNorm
    of the stored tensor itself stays inside the bound that carries the slots' fp32 error through the cancellation."""
    d, acc, dacc, gamma, beta = R.offset_case(mode, offset, conv_ref_acc(mode))
    ref = R.conv_epilogue(acc, dacc, d, mode)["out"]
    got = emu_conv(d, mode)["out"]
    assert worst(got, *ref) <= 1.0
    sv, sb = R.slot_stats(got, "tile")
    st = emu_slot_stats(got, "tile")
    assert worst(st, sv, sb) <= 1.0
    k = R.gn_finalize(sv, None, gamma, beta, R.GN_EPS, 1024, dst1=sb)
    ab, _ = emu_gn_finalize(st, None, gamma, beta, R.GN_EPS, 1024)
    e = lambda t: t[:, None, None, :]
    err = ((e(ab[..., 0]) - e(k["a"])) * got + e(ab[..., 1]) - e(k["b"])).abs()
    assert (err <= R.normalised_bound(got, k)).all(), (offset, (err / R.normalised_bound(got, k)).max().item())
    ex = R.gn_coeffs_exact(got, gamma, beta, R.GN_EPS)  # the one-pass fp64 reference IS the two-pass GroupNorm of the tensor
    assert (ex["a"] - k["a"]).abs().max().item() <= 1e-6 * k["a"].abs().max().item() * max(1, offset) ** 2


@functools.lru_cache(maxsize=None)
def conv_ref_acc(mode):
    d = R.conv_inputs(R.OFFSET_BASE, mode)
    return (d,) + R.conv_acc(d, mode)


@pytest.mark.parametrize("offset", R.GN_OFFSETS)
@pytest.mark.parametrize("case", R.GN_SYNTH, ids=lambda c: "-".join(map(str, c)))
def test_gn_finalize_emulation_and_bound(case, offset):
    d = R.gn_synth_inputs(case, offset)
    k = R.gn_finalize(d["st1"], d["st2"], d["gamma"], d["beta"], R.GN_EPS, d["hw"])
    ab, mr = emu_gn_finalize(d["st1"], d["st2"], d["gamma"], d["beta"], R.GN_EPS, d["hw"])
    assert worst(ab, *k["ab"]) <= 1.0 and worst(mr, *k["mr"]) <= 1.0, (worst(ab, *k["ab"]), worst(mr, *k["mr"]))
    if offset == 0:
        assert_bound_small("gn_finalize ab", k["ab"][0], k["ab"][1], 0)


@pytest.mark.parametrize("mode", R.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("B", [1, 3])
def test_pool_stem_head_emulation_and_bound(mode, B):
    h = head_inputs(mode, B)
    v, b = R.gn_silu_pool(h["x"], h["ab"], mode)
    got = rnd_store(emu_resample(emu_pro(h["x"].to(F32), h["ab"], R.PRO_GN_SILU), R.RES_DOWN), mode).to(F64)
    assert worst(got, v, b) <= 1.0
    assert_bound_small("pool", v, b, mode)
    for mfma in (True, False):
        v, b = R.stem(h["x_t"], h["coef"][:B], h["w_stem"], h["b_stem"], mode, mfma)
        assert worst(emu_stem(h["x_t"], h["coef"][:B], h["w_stem"], h["b_stem"], mode, mfma), v, b) <= 1.0, ("stem", mfma)
        assert_bound_small("stem", v, b, mode)
        v, b = R.aux(h["x"], h["ab"], h["w_aux"], h["b_aux"], h["x_t"], h["coef"], mode, mfma)
        assert worst(emu_aux(h["x"], h["ab"], h["w_aux"], h["b_aux"], h["x_t"], h["coef"], mode, mfma), v, b) <= 1.0, ("aux", mfma)
        assert_bound_small("aux", v, b, mode if mfma else 0)


@pytest.mark.parametrize("mode", R.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_attention_emulation_and_bound(case, mode):
    d = R.attn_inputs(case, mode)
    v, b = R.attention(d["q"], d["k"], d["vt"], mode)
    assert worst(emu_attention(d["q"], d["k"], d["vt"], mode), v, b) <= 1.0
    assert_bound_small("attention", v, b, mode)


@functools.lru_cache(maxsize=None)
def merged_chain(B, mut=None):
    """The merged attention block from the op-level pieces: merge the weights, q' | v' by the 1x1 conv reference, the attention."""
    m = R.merged_inputs(B)
    (w, dw), (b, db) = R.attn_merge_weights(m["qkv_w"], m["qkv_b"], m["proj_w"], mut)
    w32, b32 = R.f32r(w), R.f32r(b)
    d = dict(src1=m["x_mid"].reshape(B, 16, 16, 256), src2=None, ab=m["ab"], pro=R.PRO_GN, res=R.RES_NONE, outmode=R.OUT_QV,
             w=w32[:, :, None, None], bias=b32)
    qv = R.conv(d, 2)
    qm, vmt = R.f32r(qv["q"][0]), R.f32r(qv["vt"][0])
    return m, (w, dw, b, db), d, qv, qm, vmt, R.attention_merged(qm, m["x_mid"], m["ab"], vmt, m["proj_b"], R.SQRT_HALF)


@pytest.mark.parametrize("B", [1, 3])
def test_merged_attention_emulation_and_bound(B):
    m, (w, dw, b, db), d, qv, qm, vmt, (v, bound) = merged_chain(B)
    Wq, Wk, Wv = (m["qkv_w"][i::3] for i in range(3))
    assert worst(R.f32r(torch.cat([Wk.t() @ Wq, m["proj_w"] @ Wv], 0)), w, dw) <= 1.0
    got = emu_attention_merged(qm, m["x_mid"], m["ab"], vmt, m["proj_b"], R.SQRT_HALF)
    assert worst(got, v, bound) <= 1.0
    assert_bound_small("merged attention", v, bound, 2)
    # the merge is the unmerged block: softmax((q . k) / 16) v projected, + proj bias + x_mid, * scale, in fp64
    xn = m["ab"][:, None, :, 0] * m["x_mid"] + m["ab"][:, None, :, 1]
    q, k, vv = (xn @ W.t() + m["qkv_b"][i::3] for i, W in enumerate((Wq, Wk, Wv)))
    P = torch.softmax(q @ k.transpose(-1, -2) / 16.0, -1)
    plain = ((P @ vv) @ m["proj_w"].t() + m["proj_b"] + m["x_mid"]) * R.SQRT_HALF
    assert (plain - v).abs().max().item() <= 1e-4 * v.abs().max().item()
    sv, sb = R.slot_stats(got.reshape(B, 16, 16, 256), "rows32")
    assert worst(emu_slot_stats(got.reshape(B, 16, 16, 256), "rows32"), sv, sb) <= 1.0


# ---- (2) the mutants -----------------------------------------------------------------------------------------------------------------------

# mutant -> (case, output) that must reject it; every mode the case runs in is checked
CONV_MUTANT_CASES = {
    "replicate_pad": ("c3_128_32_b3", "out"), "tap_flip": ("c3_256_16_b3", "out"), "concat_shift32": ("c3_384_16_b2", "out"),
    "up_index": ("c3up_512_16_b3", "out"), "down_three": ("c1down_128_16_b3", "out"), "rshift_none": ("rs_256_16_b3", "out"),
    "temb_image0": ("c3_512_8_b3", "out"), "scale_before_resid": ("c1_256_8_b3", "out"), "pair_halo": ("c3_512_8_b3", "out"),
    "subpix_phase_swap": ("sub_512_16_b3", "out"), "vt_untransposed": ("qkv_8_b3", "vt"), "qkv_no_deinterleave": ("qkv_16_b3", "k"),
}
MUT_PARAMS = [(mut, n, key, m) for mut, (n, key) in CONV_MUTANT_CASES.items() for m in R.conv_modes(n)]


@pytest.mark.parametrize("mut,name,key,mode", MUT_PARAMS, ids=[f"{a}-{b}-{R.MODE_NAME[d]}" for a, b, c, d in MUT_PARAMS])
def test_conv_mutants(mut, name, key, mode):
    d, ref = conv_ref(name, mode)
    v, b = ref[key]
    far = worst(R.conv(d, mode, mut)[key][0], v, b)
    assert far >= 5.0, (mut, name, far)


@pytest.mark.parametrize("mode", R.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("mut", ["slot_dropped", "stats_image0"])
def test_statistics_mutants(mut, mode):
    """On the slots themselves and, through gn_finalize, on the coefficients the next conv reads."""
    d, ref = conv_ref("c3_128_32_b3", mode)
    out = R.to_storage(ref["out"][0], mode)
    for layout in ("tile", "x3"):
        sv, sb = R.slot_stats(out, layout)
        mv, _ = R.slot_stats(out, layout, mut)
        assert worst(mv, sv, sb) >= 5.0, (mut, layout)
        g = torch.Generator().manual_seed(1)
        gamma, beta = R.f32r(1 + 0.5 * torch.randn(256, generator=g, dtype=F64)), R.f32r(torch.randn(256, generator=g, dtype=F64))
        k = R.gn_finalize(sv, None, gamma, beta, R.GN_EPS, 1024, dst1=sb)
        km = R.gn_finalize(mv, None, gamma, beta, R.GN_EPS, 1024)
        assert worst(km["ab"][0], *k["ab"]) >= 5.0, (mut, layout, "ab")


@pytest.mark.parametrize("mut,case", [("straddle_octet_g0", (256, 32, 128, 8, 3)), ("no_eps", (256, 8, 0, 0, 3)), ("stats_image0", (256, 8, 256, 16, 3))])
def test_gn_finalize_mutants(mut, case):
    d = R.gn_synth_inputs(case, 0)
    k = R.gn_finalize(d["st1"], d["st2"], d["gamma"], d["beta"], R.GN_EPS, d["hw"])
    km = R.gn_finalize(d["st1"], d["st2"], d["gamma"], d["beta"], R.GN_EPS, d["hw"], mut=mut)
    assert worst(km["ab"][0], *k["ab"]) >= 5.0, mut
    if mut == "straddle_octet_g0":  # cannot show at 8 or 16 channels per group: an octet never straddles there
        e = R.gn_synth_inputs((256, 8, 0, 0, 3), 0)
        args = (e["st1"], e["st2"], e["gamma"], e["beta"], R.GN_EPS, e["hw"])
        assert torch.equal(R.gn_finalize(*args, mut=mut)["ab"][0], R.gn_finalize(*args)["ab"][0])


@pytest.mark.parametrize("mode", R.MODES, ids=MODE_IDS)
def test_attention_mutants(mode):
    for case in ((64, 1, "noise"), (256, 3, "peaked")):
        d = R.attn_inputs(case, mode)
        v, b = R.attention(d["q"], d["k"], d["vt"], mode)
        assert worst(R.attention(d["q"], d["k"], d["vt"], mode, "softmax_no_scale")[0], v, b) >= 5.0, case
    # q = 0: every logit is 0 with or without the scale - the one input family that cannot reject this mutant
    d = R.attn_inputs((64, 1, "q0"), mode)
    assert torch.equal(R.attention(d["q"], d["k"], d["vt"], mode, "softmax_no_scale")[0], R.attention(d["q"], d["k"], d["vt"], mode)[0])


def test_merged_attention_mutant():
    m, (w, dw, b, db), *_, (v, bound) = merged_chain(3)
    bm = R.attn_merge_weights(m["qkv_w"], m["qkv_b"], m["proj_w"], "merged_no_wkbq")[1][0]
    assert worst(bm, b, db) >= 5.0
    assert worst(merged_chain(3, "merged_no_wkbq")[-1][0], v, bound) >= 5.0


def test_every_mutant_is_checked():
    checked = set(CONV_MUTANT_CASES) | {"slot_dropped", "stats_image0", "straddle_octet_g0", "no_eps", "softmax_no_scale", "merged_no_wkbq"}
    assert checked == set(R.MUTANTS)


# ---- (4) the entry points: plans and refusals, no GPU --------------------------------------------------------------------------------------

def plan(mode, case, ws=1, batch=None):
    ks, pro, res, outmode, c1, c2, h, B, flags = case
    p = _lib.fg_edm_conv_plan()
    rc = _lib.lib().fg_op_edm_conv_plan(mode, ks, pro, res, outmode, c1, c2, batch or B, R.src_res(res, h), h, R.conv_cout(case), ws, int("s" in flags),
                                        ctypes.byref(p))
    return rc, p.kernel, p.stat_slots


@pytest.mark.parametrize("name,mode", CONV_PARAMS, ids=CONV_IDS)
def test_conv_plan(name, mode):
    case = R.CONV_CASES[name]
    assert plan(mode, case) == (0,) + R.expected_plan(mode, case)
    if not name.startswith(("sub_", "rs_")):  # without the wave-specialised weights every call stays on conv_fused_kernel
        assert plan(mode, case, ws=0) == (0, R.K_GENERIC, {32: 8, 16: 2, 8: 1}[case[6]])
    else:
        assert plan(mode, case, ws=0)[0] == 1 and b"no kernel" in _lib.lib().fg_last_error()


def test_plan_refusals():
    base = R.CONV_CASES["c3_128_32_b3"]
    edit = lambda **kw: tuple(kw.get(k, v) for k, v in zip(("ks", "pro", "res", "outmode", "c1", "c2", "h", "B", "flags"), base))
    L = _lib.lib()
    for mode, case, why in ((3, base, b"dtype"), (0, edit(ks=5), b"ks"), (0, edit(pro=3), b"pro"), (0, edit(res=4), b"res must"), (0, edit(outmode=2), b"outmode"),
                            (0, edit(h=64), b"resolution"), (1, edit(c1=96), b"K step"), (0, edit(c1=48), b"K step"), (0, edit(B=0), b"batch"),
                            (0, edit(outmode=R.OUT_QKV), b"cout 768"), (0, edit(pro=R.PRO_GN), b"no kernel"), (0, edit(ks=1), b"no kernel"),
                            (0, edit(res=R.RES_DOWN, h=16), b"no kernel"), (1, edit(flags="rs"), b"no kernel"),
                            # 128 input channels (four K steps) with the wave-specialised weights: conv3_ws_kernel is built for 32x32 without resampling only
                            (1, edit(h=16), b"no kernel"), (1, edit(res=R.RES_UP), b"no kernel"), (0, edit(res=R.RES_SUBPIX, h=32), b"no kernel")):
        assert plan(mode, case)[0] == 1, (mode, case)
        assert why in L.fg_last_error(), (why, L.fg_last_error())
    p = _lib.fg_edm_conv_plan()
    assert L.fg_op_edm_conv_plan(0, 3, 2, 0, 0, 128, 0, 1, 32, 16, 256, 1, 0, ctypes.byref(p)) == 1 and b"source resolution" in L.fg_last_error()
    assert L.fg_op_edm_conv_plan(0, 3, 2, 0, 0, 128, 0, 1, 32, 32, 128, 1, 0, ctypes.byref(p)) == 1 and b"multiple of 256" in L.fg_last_error()
    assert L.fg_op_edm_conv_plan(0, 3, 2, 0, 0, 128, 0, 1, 32, 32, 256, 1, 0, None) == 1


P = 0x10000  # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused before a launch


def test_conv_refusals():
    L = _lib.lib()
    ok = dict(dtype=2, ks=3, pro=2, res=0, outmode=0, src1=P, c1=128, src2=None, c2=0, batch=2, hs=32, h=32, ab=P, wpack=P, wpack_ws=P, bias=P, temb=P,
              temb_stride=256, resid=None, rshift=0, scale=1.0, out=P, cout=256, stats=P, q_out=None, k_out=None, vt_out=None)
    def call(**kw):
        a = dict(ok, **kw)
        return L.fg_op_edm_conv(*[a[k] for k in ok], None)
    for kw, why in ((dict(src1=None), b"null src1"), (dict(c2=128), b"null src1"), (dict(wpack=None), b"null src1"), (dict(ab=None), b"coefficients"),
                    (dict(out=None), b"NHWC form"), (dict(q_out=P), b"NHWC form"), (dict(temb_stride=255), b"temb_stride"), (dict(temb_stride=128), b"temb_stride"),
                    (dict(rshift=1), b"rshift without"), (dict(scale=float("inf")), b"scale"), (dict(src1=P + 8), b"16-byte"), (dict(stats=P + 4), b"16-byte"),
                    (dict(temb=P + 4), b"16-byte"), (dict(outmode=1, cout=768, h=16, hs=16, ks=1, pro=1, c1=256), b"plane forms"),
                    (dict(outmode=1, cout=768, h=16, hs=16, ks=1, pro=1, c1=256, out=None, temb=None, stats=None, q_out=P, vt_out=P), b"q_out, vt_out"),
                    (dict(outmode=4, cout=512, h=16, hs=16, ks=1, pro=1, c1=256, out=None, temb=None, stats=None, q_out=P, k_out=P, vt_out=P), b"q_out, vt_out"),
                    (dict(outmode=1, cout=768, h=16, hs=16, ks=1, pro=1, c1=256, out=None, temb=None, stats=None, q_out=P, k_out=P, vt_out=P, scale=0.5), b"unscaled"),
                    (dict(res=3, hs=16, dtype=0), b"no kernel"), (dict(res=3, hs=16, wpack_ws=None), b"no kernel"), (dict(pro=1), b"no kernel"),
                    (dict(rshift=1, resid=P, wpack_ws=None), b"no kernel"), (dict(dtype=1, c1=96), b"K step"), (dict(h=24, hs=24), b"resolution")):
        assert call(**kw) == 1, kw
        assert why in L.fg_last_error(), (kw, L.fg_last_error())


def test_pack_refusals():
    L = _lib.lib()
    nbytes = L.fg_op_edm_conv_pack_bytes
    assert nbytes(0, 0, 256, 128, 3) == 256 * 128 * 9 * 4 and nbytes(1, 0, 256, 128, 3) == 256 * 128 * 9 * 2 and nbytes(2, 0, 768, 256, 1) == 768 * 256 * 4
    assert nbytes(1, 1, 256, 128, 3) == 256 * 128 * 9 * 2 and nbytes(2, 2, 256, 128, 3) == 256 * 128 * 9 * 4 and nbytes(2, 3, 256, 128, 3) == 256 * 128 * 16 * 4
    for args in ((0, 1, 256, 128, 3), (1, 1, 256, 64, 3), (1, 1, 512, 128, 3), (1, 2, 256, 128, 3), (2, 2, 256, 96, 3), (2, 3, 256, 128, 1), (0, 0, 256, 48, 3),
                 (1, 0, 256, 96, 1), (0, 0, 100, 128, 3), (0, 4, 256, 128, 3), (3, 0, 256, 128, 3), (0, 0, 256, 128, 5), (0, 0, 0, 128, 3)):
        assert nbytes(*args) == 0, args
        assert L.fg_op_edm_conv_pack(args[0], args[1], P, P, *args[2:], 0, None) == 1 and b"no layout" in L.fg_last_error()
    assert L.fg_op_edm_conv_pack(2, 2, P, P, 256, 128, 3, 1, None) == 1 and b"de-interleave" in L.fg_last_error()
    assert L.fg_op_edm_conv_pack(0, 0, P, P, 256, 128, 1, 1, None) == 1 and b"de-interleave" in L.fg_last_error()
    assert L.fg_op_edm_conv_pack(0, 0, None, P, 256, 128, 3, 0, None) == 1 and b"null" in L.fg_last_error()
    assert L.fg_op_edm_conv_pack(0, 0, P, P + 4, 256, 128, 3, 0, None) == 1 and b"aligned" in L.fg_last_error()


def test_small_op_refusals():
    L = _lib.lib()
    last = L.fg_last_error
    fin = lambda **kw: L.fg_op_edm_gn_finalize(*[dict(dict(st1=P, c1=256, s1=8, st2=None, c2=0, s2=0, gamma=P, beta=P, eps=1e-6, ab=P, mr=None, batch=2, hw=1024), **kw)[k]
                                                 for k in ("st1", "c1", "s1", "st2", "c2", "s2", "gamma", "beta", "eps", "ab", "mr", "batch", "hw")], None)
    for kw, why in ((dict(c1=8), b"c1"), (dict(c1=516), b"c1"), (dict(c1=256, c2=260), b"c1"), (dict(c1=144), b"c1"), (dict(s1=0), b"slot counts"),
                    (dict(c2=128, st2=P, s2=0), b"slot counts"), (dict(c2=128, s2=8), b"null"), (dict(batch=0), b"batch"), (dict(hw=0), b"batch"),
                    (dict(eps=-1.0), b"eps"), (dict(st1=None), b"null"), (dict(ab=None), b"null"), (dict(ab=P + 4), b"aligned")):
        assert fin(**kw) == 1 and why in last(), (kw, last())
    for args, why in (((3, P, P, P, 1, 16, 128), b"dtype"), ((0, P, P, P, 1, 16, 100), b"multiple of 8"), ((0, P, P, P, 0, 16, 128), b"batch"),
                      ((0, None, P, P, 1, 16, 128), b"null"), ((1, P + 8, P, P, 1, 16, 128), b"aligned")):
        assert L.fg_op_edm_gn_silu_pool(*args, None) == 1 and why in last(), (args, last())
    for args, why in (((3, P, P, P, P, 1, 64), b"dtype"), ((0, P, P, P, P, 1, 128), b"t 128"), ((0, P, P, P, P, 0, 64), b"batch"), ((0, P, None, P, P, 1, 64), b"null"),
                      ((0, P, P, P + 4, P, 1, 64), b"aligned")):
        assert L.fg_op_edm_attention(*args, None) == 1 and why in last(), (args, last())
    assert L.fg_op_edm_attn_merge_weights(P, P, P, P, P, 0, None) == 1 and L.fg_op_edm_attn_merge_weights(P, None, P, P, P, 256, None) == 1
    for args, why in (((P, P, P, P, P, 0.5, P, None, 0), b"batch"), ((P, P, P, P, P, float("nan"), P, None, 1), b"scale"), ((P, P, None, P, P, 0.5, P, None, 1), b"null"),
                      ((P, P + 4, P, P, P, 0.5, P, None, 1), b"aligned")):
        assert L.fg_op_edm_attention_merged(*args, None) == 1 and why in last(), (args, last())
    hb = L.fg_op_edm_head_pack_bytes
    assert hb(0, 0, 0) == 4096 * 4 and hb(0, 1, 0) == 4096 * 2 and hb(0, 2, 0) == 4096 * 4
    assert hb(1, 0, 128) == 128 * 9 * 32 * 4 and hb(1, 1, 128) == 128 * 9 * 32 * 2 and hb(1, 1, 96) == 0 and hb(1, 2, 48) == 0 and hb(2, 0, 128) == 0 and hb(0, 3, 0) == 0
    for args, why in (((3, P, P, P, P, P, P, None, 1, 32, 3), b"dtype"), ((0, P, P, P, P, P, P, None, 1, 32, 4), b"cin"), ((0, P, P, P, P, P, P, None, 1, 6, 3), b"cin"),
                      ((0, P, P, P, P, P, P, None, 0, 32, 3), b"batch"), ((0, P, P, None, P, P, P, None, 1, 32, 3), b"null"), ((0, P, P, P, P + 8, P, P, None, 1, 32, 3), b"aligned")):
        assert L.fg_op_edm_stem(*args, None) == 1 and why in last(), (args, last())
    for args, why in (((0, P, P, P, P, P, 1, 32, 3, 100), b"cout"), ((0, P, P, P, P, P, 1, 32, 16, 128), b"LDS"), ((0, P, P, P, P, P, 1, 0, 3, 128), b"res"),
                      ((0, P, P, P, None, P, 1, 32, 3, 128), b"null")):
        assert L.fg_op_edm_conv_in(*args, None) == 1 and why in last(), (args, last())
    for args, why in (((0, P, P, P, P, P, P, P, P, 1, 100, 3), b"K step"), ((1, P, P, P, P, P, P, P, P, 1, 96, 3), b"K step"), ((0, P, P, P, P, P, P, P, P, 1, 128, 33), b"cout"),
                      ((0, P, P, P, None, P, P, P, P, 1, 128, 3), b"null"), ((0, P + 8, P, P, P, P, P, P, P, 1, 128, 3), b"aligned")):
        assert L.fg_op_edm_aux_head(*args, None) == 1 and why in last(), (args, last())
    for args, why in (((0, P, P, P, P, P, P, P, 1, 32, 100, 3), b"multiple of 32"), ((0, P, P, P, P, P, P, P, 1, 32, 128, 5), b"cout"), ((0, P, P, P, P, P, P, P, 1, 32, 512, 4), b"LDS"),
                      ((0, P, P, P, P, P, P, None, 1, 32, 128, 3), b"null")):
        assert L.fg_op_edm_aux_out(*args, None) == 1 and why in last(), (args, last())
