"""The two ends of the VACE control branch per op and per ELEMENT against fp64 (fastgen_amd/csrc/wan_embed.hip through
fg_op_wan_vace_patch_embed - path 0 / 2 = the phased kernel at 96 channels, path 1 = the per-output kernel - and through
fg_wan_set_vace_context / fg_wan_vace_context_read).  Bounds are derived from the arithmetic as tests/test_gpu_wan_ti2v_ops.py derives
its own (u = 2^-24; a sum of n terms in any order is off by at most n u sum |terms| to first order, with a 1 % allowance):

Patch embedding (both forms: one fp32 fmaf chain over the K = 4 C = 384 inputs starting at the bias, rounded to bf16 once):
    |got - want| <= 2^-8 |want| + 1.01 (K + 1) u S,   S = |bias| + sum_k |w_k| |x_k|
The tiled kernel keeps the per-output kernel's chain order: the two are BIT-EQUAL, and that is asserted.

ctx_in = proj_in(pad(tokens)) (fg_wan_set_vace_context): the bf16 tokens the embedding stored (taken from the op, whose error is bounded
above) through the bf16 token GEMM with fp32 accumulation, rounded to bf16 once:
    |got - want| <= 2^-8 |want| + 1.01 (D + 1) u (|bias| + sum_k |w_k| |tok_k|),   w = bf16(proj_in.weight)
A padded row is bf16(proj_in.bias) exactly: its product is a sum of zeros."""

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks._engine import ptr
import wan_vace_ref as V

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C = 96
# two workgroups per sample row of tiles and whole tiles (B 2, Fc 2, 16 x 24: 384 tokens), and a ragged tail (B 1, Fc 3, 6 x 10: 45 tokens)
SHAPES = {"tiles": (2, 2, 16, 24), "ragged": (1, 3, 6, 10)}


def _embed(x, w, b, path):
    Bc, Cc, Fr, Hh, Ww = x.shape
    D = w.shape[0]
    out = torch.full((Bc, Fr * (Hh // 2) * (Ww // 2), D), float("nan"), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.lib().fg_op_wan_vace_patch_embed(ptr(x), ptr(w), ptr(b), ptr(out), Bc, Cc, Fr, Hh, Ww, D, path, None))
    torch.cuda.synchronize()
    return out


def _patches(x):
    """[B, C, F, H, W] -> [B, L, C * 4] in the weight's (c, py, px) order"""
    Bc, Cc, Fr, Hh, Ww = x.shape
    p = x.view(Bc, Cc, Fr, Hh // 2, 2, Ww // 2, 2).permute(0, 2, 3, 5, 1, 4, 6)
    return p.reshape(Bc, Fr * (Hh // 2) * (Ww // 2), Cc * 4)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_tiled_embedding_is_the_generic_one_bit_for_bit_and_both_meet_fp64(shape):
    Bc, Fc, Hh, Ww = SHAPES[shape]
    D = 256
    g = torch.Generator().manual_seed(500 + Fc)
    x = torch.randn(Bc, C, Fc, Hh, Ww, generator=g).cuda()
    x[:, 32:] = 1.0  # (the 64 mask channels of a real context)
    w = (torch.randn(D, C, 1, 2, 2, generator=g) * (4 * C) ** -0.5).cuda()
    b = (0.05 * torch.randn(D, generator=g)).cuda()
    tiled, generic = _embed(x, w, b, 2), _embed(x, w, b, 1)
    assert torch.isfinite(tiled).all() and torch.equal(tiled, generic) and torch.equal(tiled, _embed(x, w, b, 0))
    p64, w64 = _patches(x).double(), w.double().view(D, -1)
    want = p64 @ w64.t() + b.double()
    bound = 2.0 ** -8 * want.abs() + 1.01 * (4 * C + 1) * U * (p64.abs() @ w64.abs().t() + b.double().abs())
    for name, got in (("tiled", tiled), ("generic", generic)):
        err = (got.double() - want).abs()
        print("vace patch embedding", shape, name, "worst err / bound", float((err / bound).max()))
        assert bool((err <= bound).all()), (name, float((err / bound).max()))
    # a neighbouring channel's weights miss the bound 5 x over
    bad = p64 @ w64.view(D, C, 4).roll(1, 1).reshape(D, -1).t() + b.double()
    assert float(((bad - want).abs() / bound).max()) >= 5.0
    with pytest.raises(RuntimeError):
        _lib.check(_lib.lib().fg_op_wan_vace_patch_embed(ptr(x[:, :48].contiguous()), ptr(w), ptr(b), ptr(tiled), Bc, 48, Fc, Hh, Ww, D, 2, None))


def _straddle_case(vace_in):
    """Batch 3, video [3, 16, 2, 4, 6] (12 tokens per sample), a context of 1 frame: 6 context tokens per sample, 18 in all - ONE 32-token
    tile that crosses two sample boundaries and writes rows 0-5, 12-17, 24-29 of the padded context (out_rows = 12 > 6).  The
    cases of wan_vace_ref.case() have 480 / 288 tokens per sample: whole tiles, no tile across a boundary.  vace_in 96: the phased
    kernel; 32: the per-output kernel with padded rows."""
    sd = V.random_state_dict(V.TINY, V.SEED, vace_in=vace_in)
    g = torch.Generator().manual_seed(V.SEED + 2)
    x = torch.randn(3, 16, 2, 4, 6, generator=g)
    lat = torch.randn(3, vace_in // 3, 1, 4, 6, generator=g)
    ctx = torch.cat([lat, torch.ones(3, vace_in - vace_in // 3, 1, 4, 6)], dim=1).contiguous()
    return sd, x, {"ctx": ctx}


@pytest.mark.parametrize("ctx_frames", [5, 3, pytest.param((1, 96), id="straddle-96"), pytest.param((1, 32), id="straddle-32")])
def test_context_setter_against_fp64_and_padded_rows_are_the_bias(ctx_frames):
    from fastgen_amd.networks.VaceWan.network import VACEWan

    vace_in = V.VACE_IN
    if isinstance(ctx_frames, tuple):
        ctx_frames, vace_in = ctx_frames
        sd, x, cond = _straddle_case(vace_in)
    else:
        sd, x, _, cond, _ = V.case("full" if ctx_frames == 5 else "short")
    net = VACEWan(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=3, vace_layers=V.VACE_LAYERS,
                  vace_in_channels=vace_in)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    Bc, _, F, H, W = x.shape
    L, D = F * (H // 2) * (W // 2), 256
    ctx = cond["ctx"].cuda()
    lib = _lib.lib()
    got = torch.full((Bc, L, D), float("nan"), device="cuda")
    assert lib.fg_wan_vace_context_read(net._h, ptr(got), None) == 2  # FG_ENOTREADY: nothing is set (not even packed)
    with torch.inference_mode():
        net._prepare(x.cuda(), "x_t", ctx)
    _lib.check(lib.fg_wan_vace_context_read(net._h, ptr(got), None))
    torch.cuda.synchronize()
    w_pe, b_pe = sd["transformer.vace_patch_embedding.weight"].cuda(), sd["transformer.vace_patch_embedding.bias"].cuda()
    tok = _embed(ctx, w_pe, b_pe, 0)  # the tokens the setter's own launch stores (path 0), [B, Fc fs, D] bf16
    Lc = tok.shape[1]
    pad = torch.zeros(Bc, L, D, dtype=torch.float64, device="cuda")
    pad[:, :Lc] = tok.double()
    w_in = sd["transformer.vace_blocks.0.proj_in.weight"].cuda().bfloat16().double()
    b_in = sd["transformer.vace_blocks.0.proj_in.bias"].cuda().double()
    want = pad @ w_in.t() + b_in
    bound = 2.0 ** -8 * want.abs() + 1.01 * (D + 1) * U * (pad.abs() @ w_in.abs().t() + b_in.abs())
    err = (got.double() - want).abs()
    print("vace ctx_in", ctx_frames, "worst err / bound", float((err / bound).max()))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), float((err / bound).max())
    if Lc < L:
        bias16 = sd["transformer.vace_blocks.0.proj_in.bias"].cuda().bfloat16().float()
        assert torch.equal(got[:, Lc:], bias16.expand(Bc, L - Lc, D))
        # padding behind proj_in (zero rows) misses the bound
        assert float((b_in.abs() / bound[:, Lc:]).max()) >= 5.0
    # against the fp64 oracle's own ctx_in (fp32 weights, no bf16 tokens): the bf16 arithmetic's distance
    ref = V.WanVaceRef(sd, V.TINY, torch.float64).ctx_in(cond["ctx"], L)
    d = float((got.cpu().double() - ref).norm() / ref.norm())
    print("vace ctx_in vs oracle, relative L2", d)
    assert d < 2e-2, d  # (the project's tolerance for this network family in bf16)
    # a second context of the same shape lands in the same buffer; another frame count is a new one of the same size here
    with torch.inference_mode():
        net._prepare(x.cuda(), "x_t", (2 * ctx).contiguous())
    got2 = torch.empty_like(got)
    _lib.check(lib.fg_wan_vace_context_read(net._h, ptr(got2), None))
    torch.cuda.synchronize()
    assert not torch.equal(got2[:, :Lc], got[:, :Lc]) and torch.equal(got2[:, Lc:], got[:, Lc:])
