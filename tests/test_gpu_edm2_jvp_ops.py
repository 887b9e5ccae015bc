"""Per-op and per-block parity of the EDM2 tangent kernels against the fp64 torch.func.jvp references of tests/edm2_jvp_ref.py: the cosine
attention's derivative (fg_op_edm2_attention_jvp), the pixel norm's (fg_op_edm2_pixel_norm_jvp), the tangent convolution's operand
(fg_op_edm2_silu_operand_jvp), every Block of two networks through fg_edm2_run_block_jvp in both compute modes, and one block with a low
clip_act.  tests/test_edm2_jvp_ref.py shows on the CPU what each bound can see (one mutant per plausible kernel error)."""
import ctypes

import pytest
import torch

from fastgen_amd import _lib

import edm2_jvp_ref as J
import edm2_ops_ref as R
import edm2_ref as D
from test_gpu_edm2_ops import dev, make_net, nan_like, nchw, nhwc, ptr

pytestmark = pytest.mark.gpu


# ---- cosine attention -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.ATTN_KINDS)
@pytest.mark.parametrize("B,T,heads", J.ATTN_JVP_SHAPES)
def test_cosine_attention_jvp(B, T, heads, kind):
    """out_d against fp64 within J.mp_attention_jvp_bound; the optional primal output bit-equal to fg_op_edm2_attention, and out_d
    the same with and without it.  The fp32 CPU oracle sits at 0.001 of the bound, the mutants at 20x and more.  Measured on an
    MI355X, worst ratio: 0.0009 (T = 128, 2 heads, tiny)."""
    L = _lib.lib()
    prim, tang = J.attn_jvp_inputs(B, T, heads, kind)
    ref_d = J.mp_attention_jvp_ref([a.double() for a in prim], [a.double() for a in tang])[1]
    qkv, qkv_d = J.attn_pack(*prim).to(dev()), J.attn_pack(*tang).to(dev())
    out, out_d, only_d, fwd = (nan_like(B, T, heads * 64) for _ in range(4))
    _lib.check(L.fg_op_edm2_attention_jvp(qkv.data_ptr(), qkv_d.data_ptr(), out.data_ptr(), out_d.data_ptr(), B, T, heads, None))
    _lib.check(L.fg_op_edm2_attention_jvp(qkv.data_ptr(), qkv_d.data_ptr(), None, only_d.data_ptr(), B, T, heads, None))
    _lib.check(L.fg_op_edm2_attention(qkv.data_ptr(), fwd.data_ptr(), B, T, heads, None))
    torch.cuda.synchronize()
    assert torch.equal(out, fwd) and torch.equal(out_d, only_d)
    got = out_d.cpu().double().reshape(B, T, heads, 64).transpose(1, 2)
    assert torch.isfinite(got).all()
    r = R.ratio((got - ref_d).abs(), J.mp_attention_jvp_bound(prim, tang))
    print(f"\ncosine attention jvp B={B} T={T} heads={heads} {kind}: max err/bound {r:.4f}")
    assert r <= 1.0, r


# ---- pixel norm -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,C,down", R.PIXNORM_CASES)
def test_pixel_norm_jvp(B, H, C, down):
    """|d| <= 2^-19 (|m_d| / n + |m| (|m| . |m_d|) / (sqrt(C) |m| n^2)), the magnitudes of the two terms; in place (out_d = x_d) without
    the 2x2 mean; the all-zero pixel's tangent is x_d / 1e-4.  Measured on an MI355X, worst ratio: 0.12 (C = 768)."""
    L = _lib.lib()
    x, xd = J.pixnorm_jvp_inputs(B, H, C, down)
    ref = J.pixel_norm_jvp_ref(x.double(), xd.double(), down)
    _, mag = J.pixel_norm_jvp_formula(x.double(), xd.double(), down)
    dx, dxd = nhwc(x).to(dev()), nhwc(xd).to(dev())
    out = dxd if not down else nan_like(B, H, H, C)
    _lib.check(L.fg_op_edm2_pixel_norm_jvp(dx.data_ptr(), dxd.data_ptr(), out.data_ptr(), B, H, C, down, None))
    got = nchw(out.cpu()).double()
    assert torch.isfinite(got).all()
    assert torch.equal(dx.cpu(), nhwc(x)) and (not down or torch.equal(dxd.cpu(), nhwc(xd)))
    if B * H * H > 1:
        md = torch.nn.functional.avg_pool2d(xd.double(), 2) if down else xd.double()
        assert (got[0, :, 0, 0] - md[0, :, 0, 0] / 1e-4).abs().max() <= 2.0 ** -21 * (md[0, :, 0, 0] / 1e-4).abs().max()
    r = R.ratio((got - ref).abs(), J.PIXNORM_JVP_REL * mag)
    print(f"\npixel_norm jvp B={B} H={H} C={C} down={down}: max err/bound {r:.3f}")
    assert r <= 1.0, r


# ---- SiLU operand ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(J.SILU_CASES))
def test_silu_operand_jvp(name):
    """silu'(a x) (a x_d + a_d x) over the virtual concat at B = 3: a broadcast row, mp_cat's row and strided per-image rows with a
    strided a_d, junk wherever the kernel must not read.  |d| <= 2^-20 (1 + |a x|) (|a x_d| + |a_d x|).  Measured on an MI355X, worst
    ratio: 0.12."""
    L = _lib.lib()
    c = J.SILU_CASES[name]
    x, xd, ab, stride, off, ad = J.silu_inputs(name)
    ref, mag = J.silu_operand_ref(name)
    C1, C2, B, hw = c["C1"], c["C2"], c["B"], c["hw"]
    d = lambda t: None if t is None else t.contiguous().to(dev())  # noqa: E731
    x1, d1 = d(x[..., :C1]), d(xd[..., :C1])
    x2, d2 = (d(x[..., C1:]), d(xd[..., C1:])) if C2 else (None, None)
    dab, dad = d(ab), d(ad)
    out = nan_like(B, hw, C1 + C2)
    _lib.check(L.fg_op_edm2_silu_operand_jvp(x1.data_ptr(), ptr(x2), d1.data_ptr(), ptr(d2), C1, C2, dab.data_ptr() + 8 * off, stride,
                                             None if dad is None else dad.data_ptr() + 4 * off, stride, out.data_ptr(), B, hw, None))
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    r = R.ratio((got - ref).abs(), J.SILU_REL * mag)
    print(f"\nsilu operand jvp {name}: max err/bound {r:.3f}")
    assert r <= 1.0, r


# ---- blocks ---------------------------------------------------------------------------------------------------------------------------
def run_block_jvp(h, ws, index, x1, x1d, x2, x2d, emb, embd):
    L = _lib.lib()
    cout, rout = ctypes.c_int(), ctypes.c_int()
    _lib.check(L.fg_edm2_block_info(h, index, None, None, ctypes.byref(cout), None, ctypes.byref(rout), None))
    up = lambda t: None if t is None else nhwc(t).to(dev())  # noqa: E731
    a1, a1d, a2, a2d = up(x1), up(x1d), up(x2), up(x2d)
    e, ed = emb.float().contiguous().to(dev()), embd.float().contiguous().to(dev())
    B = x1.shape[0]
    out, out_d, plain = (nan_like(B, rout.value, rout.value, cout.value) for _ in range(3))
    c2 = 0 if a2 is None else a2.shape[-1]
    _lib.check(L.fg_edm2_run_block_jvp(h, index, a1.data_ptr(), a1d.data_ptr(), a1.shape[-1], ptr(a2), ptr(a2d), c2, e.data_ptr(), ed.data_ptr(),
                                       out.data_ptr(), out_d.data_ptr(), B, ws.data_ptr(), ws.numel(), None))
    _lib.check(L.fg_edm2_run_block(h, index, a1.data_ptr(), a1.shape[-1], ptr(a2), c2, e.data_ptr(), plain.data_ptr(), B, ws.data_ptr(),
                                   ws.numel(), None))
    torch.cuda.synchronize()
    assert torch.equal(out, plain)  # the primal of the interleaved run is fg_edm2_run_block's, bit for bit
    return nchw(out.cpu()), nchw(out_d.cpu())


def jvp_workspace(h, B):
    return torch.empty(_lib.lib().fg_edm2_jvp_workspace_bytes(h, B), dtype=torch.uint8, device=dev())


def assert_block(key, got_d, ref_d, mode):
    """The forward's per-block bounds (tests/edm2_ops_ref.py) on the tangent: the tangent convolutions are the same kernel on operands
    of the same kind."""
    assert torch.isfinite(got_d).all(), key
    d = got_d.double() - ref_d
    mx, rel = (d.abs().max() / ref_d.abs().max()).item(), (d.norm() / ref_d.norm()).item()
    print(f"\nblock jvp {mode} {key}: max|d|/max|ref| {mx:.2e} rel L2 {rel:.2e}")
    if mode == "bf16x3":
        assert mx <= R.BLOCK_MAX_REL, (key, mx)
    else:
        assert rel <= R.BLOCK_REL_L2, (key, rel)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["narrow", "small_uncond"])
def test_blocks_jvp(name, mode):
    """Every block at B = 2 through fg_edm2_run_block_jvp against torch.func.jvp of D.block in fp64, tangents in x1, x2 and emb.
    Measured on an MI355X, worst (enc.8x8_block0 both times): bf16x3 max|d| / max|ref| 7.1e-6, bf16 rel L2 3.6e-3."""
    cfg = {"narrow": D.NARROW, "small_uncond": D.SMALL_UNCOND}[name]
    B = 2
    sd = D.random_state_dict(cfg, seed=99)
    net = make_net(cfg, sd, compute_dtype=mode)
    sd64 = R.to64(sd)
    enc, dec, _, _, _ = D.layout(cfg)
    g = R.gen(100)
    E = cfg.model_channels * max(cfg.channel_mult)
    dt, h = net._engine(dev())
    ws = jvp_workspace(h, B)
    lab = None if not cfg.label_dim else torch.nn.functional.one_hot(torch.arange(B) * 3 % cfg.label_dim, cfg.label_dim).double()
    emb, emb_d = torch.func.jvp(lambda c: D.embedding(sd64, cfg, c, lab), (torch.linspace(-1.2, 0.9, B, dtype=torch.float64),),
                                (torch.tensor([0.8, -0.5], dtype=torch.float64),))
    assert emb.shape == (B, E)
    for i, b in enumerate(enc + dec):
        x1, x1d, x2, x2d = J.block_inputs(cfg, b, B, g)
        ref, ref_d = J.block_jvp_ref(sd64, b, cfg, x1, x1d, x2, x2d, emb, emb_d)
        assert ref.abs().max() < 0.9 * cfg.clip_act
        got, got_d = run_block_jvp(h, ws, i, x1, x1d, x2, x2d, emb, emb_d)
        assert_block(b.key, got_d, ref_d, mode)
    del net
    torch.cuda.empty_cache()


def test_block_jvp_low_clip():
    """clip_act = 3 on SMALL_UNCOND's 8x8 attention block (bf16x3): the tangent is zero exactly where the oracle's primal clamps,
    and the whole tangent - nothing excluded - meets the per-block bound.  The inputs keep every fp64 pre-clamp value 100x the forward
    bound away from +-clip (asserted), so the mask the kernel takes from its own rounded output is the oracle's.  Measured on an MI355X:
    max|d| / max|ref| 6.6e-6."""
    c = J.low_clip_case()
    pre, pre_d = c["pre"], c["pre_d"]
    assert ((pre.abs() - J.LOW_CLIP).abs().min() / pre.abs().max()).item() > J.LOW_CLIP_MARGIN
    ref_d = J.clamp_jvp(pre, pre_d, J.LOW_CLIP)
    net = make_net(c["cfg"], c["sd"], compute_dtype="bf16x3")
    dt, h = net._engine(dev())
    ws = jvp_workspace(h, J.LOW_CLIP_B)
    got, got_d = run_block_jvp(h, ws, J.LOW_CLIP_BLOCK, c["x1"], c["x1d"], None, None, c["emb"], c["embd"])
    clamped = pre.abs() >= J.LOW_CLIP
    assert clamped.sum() >= 4 and torch.equal(got_d == 0, clamped) and torch.equal(got.abs() == J.LOW_CLIP, clamped)
    assert_block(c["b"].key + " clip 3", got_d, ref_d, "bf16x3")
