"""The image-to-video kernels per op (fastgen_amd/csrc/wan_i2v.hip, the concat view of wan_embed.hip) against fp64.

Dual cross-attention (fg_op_wan_dual_cross_attention), per ELEMENT: |got - want| <= bound(text) + bound(image) + U (A_txt + A_img) with
tests/token_attention_ref.py's `bound` per context (derived there, not measured) and the last term for the kernel's sum: it rounds each
context's output to bf16 (inside `bound`), adds the two in fp32 and rounds the sum once more, |sum| <= A_txt + A_img.  Headroom as in
tests/test_gpu_token_attention.py: max |err| / (2^-9 (A_txt + A_img)); 4 is the bf16 part of the bound (3 per context and the sum's rounding).
Measured on the MI355X (headroom per shape of SHAPES, in order): 2.26, 2.10, 2.89, 2.65 (worst error / bound 0.54, 0.49, 0.69, 0.63);
selection inputs exact.

Patch embedding: bit-equal to the plain network's kernel on the concatenated tensor, and inside TOK_ULP / TOK_ABS of fp64 (measured worst
error / bound 0.98).

fg_wan_i2v_cond_read: image tokens, k_img, v_img against the fp64 pieces of tests/wan_i2v_ref.py on the bf16-rounded GEMM weights, as
max |got - want| / max |want|.  Bound COND_BOUND = twice the worst measured on the MI355X over image_len {257, 1} x image_dim {128, 1280}
(D 256): measured img_tokens 5.6e-3, k_img 6.1e-3, v_img 5.1e-3 (the worst at image_len 257, image_dim 1280; every stage - LayerNorm,
hidden, GELU, output, LayerNorm, projections - stores bf16).  Mutants, each at least 5 x the bound away: norm_added_k missing, the neighbour sample's image;
the tanh GELU is REPORTED only - it does not separate (measured 2.2e-4 from the erf form on these inputs, far below the bound).
That a second fg_wan_set_i2v_cond at the same shapes keeps the buffers where they are is checked where it matters, by the graph hit of
tests/test_gpu_wan_i2v.py (the graph's key holds their addresses)."""
import ctypes

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks._engine import ptr

import token_attention_ref as TR
import wan_i2v_ref as I
from oracle import wan_ref as R

pytestmark = pytest.mark.gpu

HD = 128
SHAPES = [(1, 2, 105, 37, 257), (2, 2, 480, 512, 257), (9, 3, 128, 77, 1), (1, 40, 256, 512, 33)]  # B, H, Lq, L_txt, L_img
COND_BOUND = 2 * 6.1e-3
TOK_ULP, TOK_ABS = 2.0 ** -8, 2e-5  # tests/test_gpu_wan_blocks.py's: half a bf16 ulp of the stored value + the fp32 dot product


def _kv(k, v, pad_rows=0):
    """interleaved k|v [B, L + pad, 2 D] as the engine stores it; the padding rows are NaN: nothing may read them"""
    B, L, D = k.shape
    kv = torch.full((B, L + pad_rows, 2 * D), float("nan"), dtype=torch.bfloat16, device=k.device)
    kv[:, :L, :D], kv[:, :L, D:] = k, v
    return kv


def _dual(q, kt, vt, ki, vi, H):
    B, Lq, D = q.shape
    kvt = _kv(kt, vt)
    out = torch.full_like(q, float("nan"))
    if ki is None:
        args = (None, None, 0, 0, 0)
        kvi = None
    else:
        Li = ki.shape[1]
        kvi = _kv(ki, vi, pad_rows=(-Li) % 32)
        args = (ptr(kvi), ctypes.c_void_p(kvi.data_ptr() + 2 * D), 2 * D, kvi.shape[1] * 2 * D, Li)
    _lib.check(_lib.lib().fg_op_wan_dual_cross_attention(ptr(q), D, Lq * D, ptr(kvt), ctypes.c_void_p(kvt.data_ptr() + 2 * D), 2 * D,
                                                         kvt.shape[1] * 2 * D, kt.shape[1], *args, ptr(out), D, Lq * D, B, H, Lq, None))
    torch.cuda.synchronize()
    return out


def _refs(q, kt, vt, ki, vi, H):
    rt, ri = TR.reference(q, kt, vt, H, HD), TR.reference(q, ki, vi, H, HD)
    want, A = rt["want"] + ri["want"], rt["A"] + ri["A"]
    bnd = (TR.bound(rt, HD, kt.shape[1], float(vt.float().abs().max())) + TR.bound(ri, HD, ki.shape[1], float(vi.float().abs().max())) + TR.U * A)
    return want, A, bnd


def _joint(q, kt, vt, ki, vi, H):
    return TR.reference(q, torch.cat([ki, kt], 1), torch.cat([vi, vt], 1), H, HD)["want"]


def _swap_heads(x, H):
    B, L, D = x.shape
    return x.view(B, L, H, HD).flip(2).reshape(B, L, D)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dual_attention_per_element(shape):
    B, H, Lq, Lt, Li = shape
    g = torch.Generator().manual_seed(sum(shape))
    rn = lambda *s: torch.randn(*s, generator=g).bfloat16().cuda()
    q, kt, vt, ki, vi = 2.0 * rn(B, Lq, H * HD), rn(B, Lt, H * HD), rn(B, Lt, H * HD), rn(B, Li, H * HD), rn(B, Li, H * HD)
    got = _dual(q, kt, vt, ki, vi, H)
    want, A, bnd = _refs(q, kt, vt, ki, vi, H)
    err = (got.double() - want).abs()
    print("dual attention", shape, "headroom", float((err / (TR.U * A)).max()), "worst err / bound", float((err / bnd).max()))
    assert torch.isfinite(got).all() and bool((err <= bnd).all()), float((err / bnd).max())
    # one softmax over the concatenated keys is another function: it misses the bound 5 x over
    assert float(((_joint(q, kt, vt, ki, vi, H) - want).abs() / bnd).max()) >= 5.0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dual_attention_selects_one_key_per_context(shape):
    """`selection()` per context, the text keys living in dims [0, 64) and the image keys in [64, 128) of every head so that one query
    leads in both: out[i] = v_txt[pi(i)] + v_img[pi'(i)] to one bf16 rounding, the last valid key of both contexts among them."""
    B, H, Lq, Lt, Li = shape
    nt_t, nt_i = (Lt + 31) // 32, (Li + 31) // 32
    qt, kt, vt, pt = TR.selection(B, H, HD, Lq, Lt, [(0, nt_t)], seed=1)
    qi, ki, vi, pi = TR.selection(B, H, HD, Lq, Li, [(0, nt_i)], seed=2)
    pi = pi.roll(7, dims=-1)  # (the two contexts' choices out of step)
    qi = qi.view(B, Lq, H, HD).roll(7, dims=1).reshape(B, Lq, H * HD)
    lo = (torch.arange(H * HD) % HD < 64)
    kt, qt, ki, qi = kt * lo, qt * lo, ki * ~lo, qi * ~lo
    q = (2.0 * (qt.float() + qi.float())).bfloat16()
    q, kt, vt, ki, vi = (a.cuda() for a in (q, kt, vt, ki, vi))
    rt, ri = TR.reference(q, kt, vt, H, HD), TR.reference(q, ki, vi, H, HD)
    assert float(rt["lead"].min()) > 40.0 and (Li == 1 or float(ri["lead"].min()) > 40.0)
    assert Lt - 1 in pt.flatten().tolist() and Li - 1 in pi.flatten().tolist()
    pick = lambda v, p, L: torch.gather(v.view(B, L, H, HD).permute(0, 2, 1, 3), 2, p.cuda()[..., None].expand(-1, -1, -1, HD))
    want = (pick(vt, pt, Lt).float() + pick(vi, pi, Li).float()).bfloat16().permute(0, 2, 1, 3).reshape(B, Lq, H * HD)
    got = _dual(q, kt, vt, ki, vi, H)
    assert torch.equal(got, want), float((got.float() - want.float()).abs().max())
    # mutated references on this input: the last image key dropped, the image context's heads swapped
    ref, A, bnd = _refs(q, kt, vt, ki, vi, H)
    assert bool(((got.double() - ref).abs() <= bnd).all())
    if Li > 1:
        drop = rt["want"] + TR.reference(q, ki[:, :-1], vi[:, :-1], H, HD)["want"]
        assert float(((drop - ref).abs() / bnd).max()) >= 5.0
    swapped = rt["want"] + TR.reference(q, _swap_heads(ki, H), _swap_heads(vi, H), H, HD)["want"]
    assert float(((swapped - ref).abs() / bnd).max()) >= 5.0


def test_dual_attention_without_image_keys_is_the_text_attention():
    B, H, Lq, Lt = 2, 2, 130, 64
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g).bfloat16().cuda()
    q, kt, vt = 2.0 * rn(B, Lq, H * HD), rn(B, Lt, H * HD), rn(B, Lt, H * HD)
    got = _dual(q, kt, vt, None, None, H)
    D, kv, want = H * HD, _kv(kt, vt), torch.empty_like(q)
    _lib.check(_lib.lib().fg_op_attention_ex(ptr(q), D, Lq * D, ptr(kv), ctypes.c_void_p(kv.data_ptr() + 2 * D), 2 * D, Lt * 2 * D, ptr(want), D,
                                             Lq * D, B, H, HD, Lq, Lt, 0, 0, 0, None))
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, want)
    ref = TR.reference(q, kt, vt, H, HD)
    assert bool(((got.double() - ref["want"]).abs() <= TR.bound(ref, HD, Lt, float(vt.float().abs().max()))).all())


# ---- through a handle: the patch embedding and the condition ----------------------------------------------------------------------------
KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2)


def _i2v_net(sd, image_dim, **kw):
    from fastgen_amd.networks.WanI2V.network import WanI2V

    net = WanI2V(**dict(KW, image_dim=image_dim, **kw))
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


def _tokens(net, x, text, prepare=None, out_channels=16):
    """tokens_out of fg_wan_forward_full_features on the module's handle"""
    B, _, F, H, W = x.shape
    dev, L = x.device, _lib.lib()
    if prepare:
        prepare()
    net._bind(dev)
    ws = net._ws(L.fg_wan_full_workspace_bytes(net._h, B, F, H, W), dev)
    net._set_text(text, B, dev, ws)
    ts = torch.full((B * F,), 500.0, device=dev)
    out = torch.empty(B, out_channels, F, H, W, device=dev)
    tok = torch.empty(B, F * (H // 2) * (W // 2), 256, device=dev)
    _lib.check(L.fg_wan_forward_full_features(net._h, ptr(x), ptr(ts), None, ptr(out), B, F, H, W, None, 0, None, None, 0, ptr(tok), None, None,
                                              ptr(ws), ws.numel(), None))
    torch.cuda.synchronize()
    return tok


@pytest.mark.parametrize("frames,latent", [(1, 16), (5, 16), (5, 8)])
def test_patch_embedding_is_the_plain_kernel_on_the_concatenated_tensor(frames, latent):
    """latent 16: the LDS-staged kernel (32-token tiles: 30 tokens in one ragged tile, 150 in four and a ragged one); 8: the per-output one"""
    import dataclasses

    from fastgen_amd.networks.Wan.network import Wan

    chans = dict(in_channels=2 * latent + 4, out_channels=latent)
    sd = R.random_state_dict(dataclasses.replace(R.TINY, **chans), 11)
    B, H, W = 2, 6, 10  # 15-token frames
    g = torch.Generator().manual_seed(12 + frames)
    x, ff = torch.randn(B, latent, frames, H, W, generator=g).cuda(), torch.randn(B, latent, frames, H, W, generator=g).cuda()
    text = torch.randn(B, 5, 128, generator=g).cuda()
    net = _i2v_net(sd, 0, **chans)
    plain = Wan(**dict(KW, **chans))
    plain.load_state_dict(sd, strict=True)
    plain = plain.cuda().eval()
    with torch.inference_mode():
        got = _tokens(net, x, text, prepare=lambda: net._prepare(x, "x_t", ff, None), out_channels=latent)
        cat = torch.cat([x, I.mask_first_frame(B, frames, H, W).cuda(), ff], dim=1)
        want = _tokens(plain, cat, text, out_channels=latent)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    p64 = {k[len("transformer."):]: v.double().cuda() for k, v in sd.items() if "patch_embedding" in k}
    tok = R.patch_embed(p64, I.i2v_input(x.double().cpu(), ff.double().cpu()).cuda())
    q_ = ((got.double() - tok).abs() / (TOK_ULP * tok.abs() + TOK_ABS * tok.abs().max())).max()
    print("i2v patch embedding vs fp64, worst error / bound", float(q_))
    assert float(q_) <= 1.0
    # the mask on every frame, or the first-frame latents in the mask's place, are other tokens
    for mu in ("mask_every_frame", "cond_before_mask"):
        if frames == 1 and mu == "mask_every_frame":
            continue  # (one frame: the same mask)
        bad = R.patch_embed(p64, I.i2v_input(x.double().cpu(), ff.double().cpu(), mu).cuda())
        assert float(((bad - tok).abs() / (TOK_ULP * tok.abs() + TOK_ABS * tok.abs().max())).max()) >= 5.0, mu


def _round_gemm_weights(sd):
    """the GEMM operands the engine packs to bf16, rounded; everything else fp32 as the engine keeps it"""
    names = ("image_embedder.ff.net.0.proj.weight", "image_embedder.ff.net.2.weight", "add_k_proj.weight", "add_v_proj.weight")
    return {k[len("transformer."):]: (v.bfloat16() if k.endswith(names) else v).double().cuda() for k, v in sd.items()}


@pytest.mark.parametrize("image_dim", [128, 1280])
@pytest.mark.parametrize("image_len", [257, 1])
def test_condition_read_back_against_fp64(image_len, image_dim):
    sd = I.random_state_dict(I.TINY, image_dim, 13)
    net = _i2v_net(sd, image_dim)
    B, D = 2, 256
    g = torch.Generator().manual_seed(14 + image_len)
    x = torch.zeros(B, 16, 1, 4, 4).cuda()
    img = torch.randn(B, image_len, image_dim, generator=g).cuda()
    with torch.inference_mode():
        net._prepare(x, "x_t", x, img)
    L = _lib.lib()
    p = _round_gemm_weights(sd)
    tok64 = I.image_embedding(p, img.double())
    worst = {}
    for blk in range(2):
        tok, k, v = (torch.empty(B, image_len, D, device="cuda") for _ in range(3))
        _lib.check(L.fg_wan_i2v_cond_read(net._h, blk, ptr(tok), ptr(k), ptr(v), None))
        k64, v64 = (a.reshape(B, image_len, D) for a in I.img_kv(p, I.TINY, blk, tok64))
        rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
        for name, a, b in (("img_tokens", tok, tok64), ("k_img", k, k64), ("v_img", v, v64)):
            worst[name] = max(worst.get(name, 0.0), rel(a, b))
        # mutants: no norm_added_k; sample b sees sample b + 1's image
        k_nonorm = I.img_kv(p, I.TINY, blk, tok64, norm=False)[0].reshape(B, image_len, D)
        assert rel(k, k_nonorm) >= 5 * COND_BOUND
        for a, b in ((tok, tok64), (k, k64), (v, v64)):
            assert rel(a, b.roll(-1, 0)) >= 5 * COND_BOUND
        tanh = I.image_embedding(p, img.double(), gelu="tanh")
        print("  tanh-GELU image tokens vs erf (reported, not a separating mutant):", rel(tanh, tok64))
    print("cond read-back", image_len, image_dim, worst)
    assert all(v <= COND_BOUND for v in worst.values()), worst
