"""The two ends of the video DiT per op and per ELEMENT against fp64 (fastgen_amd/csrc/wan_embed.hip through fg_op_wan_patch_embed and
wan_ti2v.hip through fg_op_wan_final; path 0 / 2 = the tiled 48-channel kernels, path 1 = the per-output embedding and the wave-per-token
head of wan.hip).
Bounds are derived from the arithmetic, not measured (u = 2^-24, the unit roundoff of fp32; a sum of n terms in any order is off by at
most n u sum |terms| to first order, taken with a 1 % allowance for the higher orders):

Patch embedding (both forms: one fp32 fmaf chain over the K = 4 C inputs starting at the bias, rounded to bf16 once):
    |got - want| <= 2^-8 |want| + 1.01 (K + 1) u S,   S = |bias| + sum_k |w_k| |x_k|
(half a bf16 ulp - 8 significant bits - of the stored value, and the chain's error, which may also move the value across a rounding boundary: covered by the 1 %).
The tiled kernel keeps the per-output kernel's chain order: the two are BIT-EQUAL, and that is asserted.

Output head (bf16 tokens x, fp32 everything else).  With n = (x - mean) rstd, y = n (1 + scale) + shift, A = mean |x|:
  * mean: every lane adds D / 64 values, six shuffle steps join the lanes: |mean^ - mean| <= (D / 64 + 7) u A =: dm;
  * rstd: the same sum over squares that carry 3 u each, then 1 / sqrt: relative error <= (D / 128 + 8) u (dm enters squared);
  * y^ = fmaf((x - mean^) rstd^, 1 + scale, shift): |y^ - y| <= e1 |n (1 + scale)| + dm rstd |1 + scale| + u |y|, e1 = (D / 128 + 12) u;
  * the dot product over D and the bias: (D + 1) u (sum_k |y_k w_k| + |bias|), whatever the order (chain, or lanes and shuffles).
    |got - want| <= sum_k |w_k| (e1 |n_k (1 + scale_k)| + dm rstd |1 + scale_k| + u |y_k|) + 1.01 (D + 1) u (sum_k |y_k w_k| + |bias|)
Frame 0 with the second source is that source's copy, bit for bit, and frame 0's tokens depend on the second source alone.
Measured on the MI355X, worst error / bound: patch embedding 0.96 - 0.98 at every width (the bf16 rounding is the bound's main term and
some element always lands half an ulp off); head 1.0e-3 - 1.2e-2 (tiled kernel), 1.0e-4 - 3.0e-3 (wave-per-token head): worst-case
bounds over D terms against errors that add up like a random walk."""
import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks._engine import ptr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
B, FR, H, W = 2, 2, 6, 10  # 15 tokens per frame, 60 in all: ragged against the 32-token tiles, two workgroups
WIDTHS = (256, 384, 3072)
EPS = 1e-6


def _embed(x, ff, w, b, path=0):
    Bc, C, Fr, Hh, Ww = x.shape
    D = w.shape[0]
    out = torch.full((Bc, Fr * (Hh // 2) * (Ww // 2), D), float("nan"), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.lib().fg_op_wan_patch_embed(ptr(x), ptr(ff), ptr(w), ptr(b), ptr(out), Bc, C, Fr, Hh, Ww, D, path, None))
    torch.cuda.synchronize()
    return out


def _final(tok, mod, w, b, ff, C, path=0):
    D = tok.shape[-1]
    out = torch.full((B, C, FR, H, W), float("nan"), device=tok.device)
    _lib.check(_lib.lib().fg_op_wan_final(ptr(tok), ptr(mod), ptr(w), ptr(b), ptr(ff), ptr(out), B, C, FR, H // 2, W // 2, D, EPS, path, None))
    torch.cuda.synchronize()
    return out


def _replaced(x, ff):
    y = x.clone()
    y[:, :, 0] = ff[:, :, 0]
    return y


def _patches(x):
    """[B, C, F, H, W] -> [B, L, C * 4] in the weight's (c, py, px) order"""
    Bc, C, Fr, Hh, Ww = x.shape
    p = x.view(Bc, C, Fr, Hh // 2, 2, Ww // 2, 2).permute(0, 2, 3, 5, 1, 4, 6)
    return p.reshape(Bc, Fr * (Hh // 2) * (Ww // 2), C * 4)


def _embed_case(C, D, seed):
    g = torch.Generator().manual_seed(seed)
    x, ff = torch.randn(B, C, FR, H, W, generator=g).cuda(), torch.randn(B, C, 1, H, W, generator=g).cuda()
    w = (torch.randn(D, C, 1, 2, 2, generator=g) * (4 * C) ** -0.5).cuda()
    return x, ff, w, (0.05 * torch.randn(D, generator=g)).cuda()


@pytest.mark.parametrize("with_ff", [False, True], ids=["plain", "first_frame"])
@pytest.mark.parametrize("D", WIDTHS)
def test_patch_embedding_48_per_element(D, with_ff):
    C = 48
    x, ff, w, b = _embed_case(C, D, 100 + D)
    src = ff if with_ff else None
    got = _embed(x, src, w, b, 2)
    assert torch.isfinite(got).all()
    assert torch.equal(got, _embed(x, src, w, b, 0))  # (what the engine launches at 48 channels)
    xin = _replaced(x, ff) if with_ff else x
    p64, w64 = _patches(xin).double(), w.double().view(D, -1)
    want = p64 @ w64.t() + b.double()
    S = p64.abs() @ w64.abs().t() + b.double().abs()
    bound = 2.0 ** -8 * want.abs() + 1.01 * (4 * C + 1) * U * S
    err = (got.double() - want).abs()
    print("patch embedding 48", D, with_ff, "worst err / bound", float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())
    # the same chain as the per-output kernel's: bit-equal to it (on the materialised input when there is a second source)
    assert torch.equal(got, _embed(xin, None, w, b, 1))
    assert torch.equal(got, _embed(x, src, w, b, 1))
    if with_ff:
        # frame 0's tokens depend on the second source alone; the others do not see it
        x2 = x.clone()
        x2[:, :, 0] = 7.0
        assert torch.equal(_embed(x2, ff, w, b, 2), got)
        other = _embed(x, ff.roll(1, 0), w, b, 2).view(B, FR, -1, D)
        g4 = got.view(B, FR, -1, D)
        assert torch.equal(other[:, 1:], g4[:, 1:]) and not torch.equal(other[:, 0], g4[:, 0])
        assert float(((other.double().view_as(want) - want).abs() / bound).max()) >= 5.0  # the neighbour's first frame misses the bound


@pytest.mark.parametrize("C", [16, 20])
def test_patch_embedding_other_channel_counts_run_the_untouched_kernels(C):
    D = 256
    x, ff, w, b = _embed_case(C, D, 200 + C)
    plain = _embed(x, None, w, b, 0)
    assert torch.isfinite(plain).all() and torch.equal(plain, _embed(x, None, w, b, 1))
    want = _patches(x).double() @ w.double().view(D, -1).t() + b.double()
    S = _patches(x).double().abs() @ w.double().view(D, -1).abs().t() + b.double().abs()
    assert bool(((plain.double() - want).abs() <= 2.0 ** -8 * want.abs() + 1.01 * (4 * C + 1) * U * S).all())
    # with the second source: the untouched kernel's result on the materialised input, bit for bit
    assert torch.equal(_embed(x, ff, w, b, 0), _embed(_replaced(x, ff), None, w, b, 0))
    with pytest.raises(RuntimeError):
        _embed(x, None, w, b, 2)  # the tiled kernel serves 48 channels


def _final_case(C, D, seed):
    g = torch.Generator().manual_seed(seed)
    L = FR * (H // 2) * (W // 2)
    tok = (torch.randn(B * L, D, generator=g) * 1.5 + 0.3).bfloat16().cuda()
    mod = (0.5 * torch.randn(B * FR, 2, D, generator=g)).cuda()
    w = (torch.randn(4 * C, D, generator=g) * D ** -0.5).cuda()
    return tok, mod, w, (0.05 * torch.randn(4 * C, generator=g)).cuda(), torch.randn(B, C, 1, H, W, generator=g).cuda()


def _final_ref(tok, mod, w, b, C):
    """(want [B, C, F, H, W], bound) in fp64"""
    D = tok.shape[-1]
    gh, gw = H // 2, W // 2
    x = tok.double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + EPS)
    m = mod.double().repeat_interleave(gh * gw, dim=0)  # [B L, 2, D]
    sc1 = 1.0 + m[:, 1]
    n = (x - mean) * rstd
    y = n * sc1 + m[:, 0]
    w64, b64 = w.double(), b.double()
    want = y @ w64.t() + b64
    A = x.abs().mean(-1, keepdim=True)
    dm, e1 = (D / 64 + 7) * U * A, (D / 128 + 12) * U
    dy = e1 * (n * sc1).abs() + dm * rstd * sc1.abs() + U * y.abs()
    bound = dy @ w64.abs().t() + 1.01 * (D + 1) * U * (y.abs() @ w64.abs().t() + b64.abs())
    unp = lambda o: o.view(B, FR, gh, gw, 1, 2, 2, C).permute(0, 7, 1, 4, 2, 5, 3, 6).reshape(B, C, FR, H, W)
    return unp(want), unp(bound)


@pytest.mark.parametrize("with_ff", [False, True], ids=["plain", "first_frame"])
@pytest.mark.parametrize("D", WIDTHS)
def test_final_48_per_element(D, with_ff):
    C = 48
    tok, mod, w, b, ff = _final_case(C, D, 300 + D)
    want, bound = _final_ref(tok, mod, w, b, C)
    src = ff if with_ff else None
    for path in (2, 1):  # the tiled kernel, and the wave-per-token head on the same inputs
        got = _final(tok, mod, w, b, src, C, path)
        assert torch.isfinite(got).all()
        lo = 1 if with_ff else 0
        err = (got.double() - want).abs()[:, :, lo:]
        print("final 48", D, with_ff, "path", path, "worst err / bound", float((err / bound[:, :, lo:]).max()))
        assert bool((err <= bound[:, :, lo:]).all()), float((err / bound[:, :, lo:]).max())
        if with_ff:
            assert torch.equal(got[:, :, 0], ff[:, :, 0])
    assert torch.equal(_final(tok, mod, w, b, src, C, 0), _final(tok, mod, w, b, src, C, 2))
    # another frame's modulation row, or the shift and scale rows swapped, miss the bound 5 x over
    for bad_mod in (mod.roll(1, 0), mod.flip(1)):
        bad = _final_ref(tok, bad_mod, w, b, C)[0]
        assert float(((bad - want).abs() / bound).max()) >= 5.0


def test_final_16_is_the_existing_head():
    C, D = 16, 256
    tok, mod, w, b, ff = _final_case(C, D, 400)
    want, bound = _final_ref(tok, mod, w, b, C)
    got = _final(tok, mod, w, b, None, C, 0)
    assert torch.isfinite(got).all() and torch.equal(got, _final(tok, mod, w, b, None, C, 1))
    assert bool(((got.double() - want).abs() <= bound).all())
    rep = _final(tok, mod, w, b, ff, C, 0)
    assert torch.equal(rep[:, :, 0], ff[:, :, 0]) and torch.equal(rep[:, :, 1:], got[:, :, 1:])
    with pytest.raises(RuntimeError):
        _final(tok, mod, w, b, None, C, 2)
