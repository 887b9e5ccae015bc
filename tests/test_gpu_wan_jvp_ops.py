"""The kernels `fg_wan_jvp` adds (fastgen_amd/csrc/wan_jvp.hip), each on its own through its `fg_op_wan_*_jvp` entry point against the
fp64 mirror tests/wan_jvp_ref.py (pinned on the CPU by tests/test_wan_jvp_ref.py) on the values the kernel reads (bf16-exact inputs),
per token row or per (sample, query, head).  Slack rows inside the test's own allocations hold NaN: behind the tokens, behind the keys
(the `kv_bs > Lkv * ldk` layout) and behind the outputs, where they must still stand afterwards.

Attention (heads 2 unless named, head dim 128; J.ATT_CASES): one ragged tile (105 keys: waves without rows, a 9-key last tile), many
tiles (555, 3 heads: five query tiles, 18 key tiles of rescaling), long (1152 keys; the fp64 reference runs on the device), cross
(105 x 37, interleaved k | v rows, null kd / vd), vd only (qd = kd = 0: Od = P vd), no vd, and the common shift: kd plus one row common
to all keys, J.COMMON_SHIFT times the size of the rest (tests/test_wan_jvp_ref.py::test_common_shift_ratio) - its Od must hold the
bound the un-shifted cases set.  The self-attention cases read packed q | k | v rows.  The kernel's primal O is held to the existing
attn1 and attn1/row bounds of tests/test_gpu_wan_blocks.py; it is NOT bit-equal to fg_op_attention_ex's and no such thing is asserted:
that launcher picks among kernels with other summation orders (key splits with a merge pass, fa2_kernel's eras of the running maximum),
this kernel walks the keys once in tiles of 32.

Every row of Od is also held against its own size plus the size at which the kernel rounds W, |c_i - delta_i| |v| (J.ATT_TOL's
"od/row-scaled"): one bound for every case, the cross-attention's null kd / vd included.

Bounds (J.ATT_TOL, OP_TOL below): twice the worst value measured on an MI355X over each matrix, as TOL in tests/test_gpu_wan_blocks.py.
Mutants: (a) drop_delta and (b) drop_pvd on the attention, (d) drop_mod on the modulate and the output layer, (e) drop_proj on the
RMSNorm - each must miss its bound MUTANT_FACTOR times over in its closest sample."""
import ctypes
import types

import pytest
import torch

import wan_jvp_ref as J
from fastgen_amd import _lib
from oracle import wan_ref as R
from test_gpu_wan_blocks import MUTANT_FACTOR, TOL

pytestmark = pytest.mark.gpu
assert MUTANT_FACTOR == J.MUTANT_FACTOR

NAN = float("nan")
# (relative L2, max |err| / max |ref|) per token row (per sample for `final`: an output pixel sums one token), primal and tangent,
# = twice the worst measured on an MI355X over GRIDS x WIDTHS (the case that set each): modulate y 2.24e-3 (5x96 D256) / 3.83e-3
# (7x15 D1536), yd 2.12e-3 / 3.85e-3 (5x96 D256); rms_rope n 2.05e-3 (7x15 D256) / 3.86e-3 (5x96 D1536), nd 2.03e-3 (5x96 D256) /
# 3.77e-3 (5x96 D384); gelu a 1.54e-3 / 1.75e-3, ad 1.91e-3 / 3.84e-3 (5x96); final out 1.32e-7 / 1.87e-7 (5x96 D1536), jvp 1.27e-7
# (5x96 D1536) / 1.68e-7 (5x96 D384).  The bf16 stores round by 2^-9 / sqrt(3) of an element on average and 2^-8 at worst; the output
# layer writes fp32.  Mutants, closest sample as a multiple of the tangent's bound: drop_mod 520 (modulate) and 5.6e6 (final);
# drop_proj 125 (xd carries a part along x, see test_rms_rope_jvp).
OP_TOL = {"mod": (4.5e-3, 7.7e-3), "mod_d": (4.3e-3, 7.7e-3), "rms": (4.2e-3, 7.8e-3), "rms_d": (4.1e-3, 7.6e-3), "gelu": (3.1e-3, 3.6e-3),
          "gelu_d": (3.9e-3, 7.7e-3), "final": (2.7e-7, 3.8e-7), "final_d": (2.6e-7, 3.4e-7)}
GRIDS = {"7x15": (2, 7, 5, 3), "5x96": (2, 5, 8, 12)}  # B, frames, gh, gw
WIDTHS = (256, 384, 1536)


def dev():
    return torch.device("cuda:0")


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def _err(got, ref, dims):
    e = got - ref
    return e.pow(2).sum(dims).sqrt() / ref.pow(2).sum(dims).sqrt(), e.abs().amax(dims) / ref.abs().amax(dims)


def _hold(tag, got, ref, dims, tol, bad):
    rel, mx = _err(got, ref, dims)
    print(f"[wan-jvp-ops] {tag}: {float(rel.max()):.3e} / {float(mx.max()):.3e}  (bound {tol[0]:.2e} / {tol[1]:.2e})")
    if not (bool((rel <= tol[0]).all()) and bool((mx <= tol[1]).all())):  # (NaN fails)
        bad.append((tag, float(rel.max()), float(mx.max())))


def _mutant(tag, got, mref, tol, bad):
    d = float(J.rel_l2(got, mref).min())
    print(f"[wan-jvp-ops] {tag}: closest sample {d:.3e} = {d / tol[0]:.1f} x bound")
    if not d >= MUTANT_FACTOR * tol[0]:
        bad.append((tag, "mutant not seen", d / tol[0]))


def _padded(v, rows_extra):
    """[B, L, W] fp64 -> bf16 device tensor [B, L + rows_extra, W] with NaN in the slack rows."""
    B, L, Wd = v.shape
    t = torch.full((B, L + rows_extra, Wd), NAN, dtype=torch.bfloat16, device=dev())
    t[:, :L] = v.to(dev()).to(torch.bfloat16)
    return t


# ---- attention --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(J.ATT_CASES))
def test_attention_jvp(name):
    c = J.ATT_CASES[name]
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    D = 128 * H
    odev = dev() if Lq > 600 else "cpu"
    q, k, v, qd, kd, vd = J.att_case(name, odev)
    fl = lambda a: a.flatten(2)  # noqa: E731
    SL = 5  # slack rows behind every sample's tokens / keys
    out = torch.full((B, Lq + SL, D), NAN, dtype=torch.bfloat16, device=dev())
    outd = torch.full_like(out, NAN)
    L = _lib.lib()
    if c.get("cross"):
        qt, qdt = _padded(fl(q), SL), _padded(fl(qd), SL)
        kv = _padded(torch.cat([fl(k), fl(v)], -1), SL)  # interleaved k | v rows
        _lib.check(L.fg_op_wan_attention_jvp(_p(qt), _p(qdt), D, (Lq + SL) * D, _p(kv), _p(kv, D), None, None, 2 * D, (Lk + SL) * 2 * D, _p(out),
                                             _p(outd), D, (Lq + SL) * D, B, H, Lq, Lk, _stream()))
    else:
        qkv = _padded(torch.cat([fl(q), fl(k), fl(v)], -1), SL)  # packed q | k | v rows, Lq == Lk
        qkvd = _padded(torch.cat([fl(qd), fl(kd), fl(vd)], -1), SL)
        bs = (Lq + SL) * 3 * D
        _lib.check(L.fg_op_wan_attention_jvp(_p(qkv), _p(qkvd), 3 * D, bs, _p(qkv, D), _p(qkv, 2 * D), _p(qkvd, D), _p(qkvd, 2 * D), 3 * D, bs,
                                             _p(out), _p(outd), D, (Lq + SL) * D, B, H, Lq, Lk, _stream()))
    torch.cuda.synchronize()
    assert bool(out[:, Lq:].isnan().all()) and bool(outd[:, Lq:].isnan().all()), "a slack row of the outputs was written"
    o, od = (t[:, :Lq].double().to(odev).view(B, Lq, H, 128) for t in (out, outd))
    want, wantd = (t.view(B, Lq, H, 128) for t in J.attention_jvp(q, k, v, qd, kd, vd))
    bad = []
    _hold(f"attention {name} O per (sample, query, head)", o, want, (3,), TOL["attn1/row"], bad)
    _hold(f"attention {name} O per (sample, head)", o, want, (1, 3), TOL["attn1"], bad)
    if vd is not None and bool(vd.any()):  # (without the P vd term a row of Od can be arbitrarily small: the scaled check below holds it)
        _hold(f"attention {name} Od per (sample, query, head)", od, wantd, (3,), J.ATT_TOL["od/row"], bad)
    _hold(f"attention {name} Od per (sample, head)", od, wantd, (1, 3), J.ATT_TOL["od"], bad)
    # ... and every row, of every case, against its own size plus the size at which the kernel rounds W = P (Sd - c_i): |c_i - delta_i| |v|
    den = wantd.norm(dim=3) + J.attention_ref_distance(q, k, qd, kd) * v.pow(2).sum(-1).mean(1).sqrt()[:, None, :]
    scaled = float(((od - wantd).norm(dim=3) / den).max())
    print(f"[wan-jvp-ops] attention {name} Od per (sample, query, head), scaled: {scaled:.3e}  (bound {J.ATT_TOL['od/row-scaled']:.2e})")
    if not scaled <= J.ATT_TOL["od/row-scaled"]:
        bad.append((f"attention {name} Od scaled", scaled))
    for m in ("drop_delta", "drop_pvd"):
        if (m == "drop_pvd" and vd is None) or name in J.ATT_MUTANT_SKIP.get(m, ()):
            continue
        _mutant(f"attention {name} {m}", od.flatten(2), J.attention_jvp(q, k, v, qd, kd, vd, **{m: True})[1], J.ATT_TOL["od"], bad)
    assert not bad, bad


# ---- LayerNorm-modulate, RMSNorm + RoPE, GELU, output layer ---------------------------------------------------------------------------------
def _tokens(B, L, D, seed, big=100.0):
    """x (around 0.3, spread 2) and xd (spread `big`: a tangent under the x1000 timestep scale), bf16-exact fp64 [B, L, D]."""
    g = torch.Generator().manual_seed(seed)
    return J.bf16_exact(2.0 * torch.randn(B, L, D, generator=g) + 0.3), J.bf16_exact(big * torch.randn(B, L, D, generator=g))


def _mod_rows(B, Fr, n, D, seed, big=100.0):
    """Every frame its own rows: mod (spread 0.5) and modd (spread `big`) [B, F, n, D], fp32-exact fp64."""
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(B, Fr, n, D, generator=g)).double(), (big * torch.randn(B, Fr, n, D, generator=g)).double()


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_modulate_jvp(grid, D):
    B, Fr, gh, gw = GRIDS[grid]
    fs = gh * gw
    Ltok = Fr * fs
    x, xd = _tokens(B, Ltok, D, 11 + D)
    mod, modd = _mod_rows(B, Fr, 6, D, 12 + D)
    xt, xdt = _padded(x.reshape(1, B * Ltok, D), 3), _padded(xd.reshape(1, B * Ltok, D), 3)
    y = torch.full_like(xt, NAN)
    yd = torch.full_like(xt, NAN)
    mg, mdg = mod.float().to(dev()).contiguous(), modd.float().to(dev()).contiguous()
    bad = []
    for so, co, tag in ((0, D, "attn rows"), (3 * D, 4 * D, "mlp rows")):
        _lib.check(_lib.lib().fg_op_wan_modulate_jvp(_p(xt), _p(xdt), _p(mg), _p(mdg), 6 * D, so, co, _p(y), _p(yd), B * Ltok, D, fs, 1e-6, _stream()))
        torch.cuda.synchronize()
        assert bool(y[:, B * Ltok:].isnan().all()) and bool(yd[:, B * Ltok:].isnan().all())
        row = lambda m, j: J.per_frame_rows(m[:, :, j], Ltok)  # noqa: E731
        args = (x, xd, row(mod, co // D), row(mod, so // D), row(modd, co // D), row(modd, so // D), 1e-6)
        want, wantd = J.ln_modulate_jvp(*args)
        got, gotd = (t[0, :B * Ltok].double().cpu().view(B, Ltok, D) for t in (y, yd))
        _hold(f"modulate {grid} D{D} {tag} y", got, want, (2,), OP_TOL["mod"], bad)
        _hold(f"modulate {grid} D{D} {tag} yd", gotd, wantd, (2,), OP_TOL["mod_d"], bad)
        _mutant(f"modulate {grid} D{D} {tag} drop_mod", gotd, J.ln_modulate_jvp(*args, drop_mod=True)[1], OP_TOL["mod_d"], bad)
    # the cross-attention norm: a constant affine (null modd, one row for every token)
    n2 = torch.cat([mod[0, 0, 0], mod[0, 0, 1]]).float().to(dev()).contiguous()
    _lib.check(_lib.lib().fg_op_wan_modulate_jvp(_p(xt), _p(xdt), _p(n2), None, 0, 0, D, _p(y), _p(yd), B * Ltok, D, B * Ltok, 1e-6, _stream()))
    zero = torch.zeros((), dtype=torch.float64)
    want, wantd = J.ln_modulate_jvp(x, xd, mod[0, 0, 1], mod[0, 0, 0], zero, zero, 1e-6)
    got, gotd = (t[0, :B * Ltok].double().cpu().view(B, Ltok, D) for t in (y, yd))
    _hold(f"modulate {grid} D{D} constant affine y", got, want, (2,), OP_TOL["mod"], bad)
    _hold(f"modulate {grid} D{D} constant affine yd", gotd, wantd, (2,), OP_TOL["mod_d"], bad)
    assert not bad, bad


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_rms_rope_jvp(grid, D):
    B, Fr, gh, gw = GRIDS[grid]
    Ltok, H = Fr * gh * gw, D // 128
    cfg = R.WanConfig(num_heads=H, head_dim=128, rope_max_seq_len=max(Fr, gh, gw))
    x3, x3d = _tokens(B, Ltok, 3 * D, 21 + D)  # packed q | k | v rows: the kernel reads the k columns
    # (a part of xd along x: the projection term the mutant drops is otherwise 1 / sqrt(D) of the tangent - 4.8 bounds at D 1536)
    x3d = J.bf16_exact(x3d + 30.0 * x3)
    x, xd = x3[..., D:2 * D], x3d[..., D:2 * D]
    w = (1 + 0.2 * torch.randn(D, generator=torch.Generator().manual_seed(22))).double()
    cos, sin = R.rope_for_chunk(cfg, Fr, gh, gw, 0, torch.float64)
    cs = torch.stack([cos[:, 0::2], sin[:, 1::2]], -1).float().to(dev()).contiguous()  # [L][64] {cos, sin}
    xt, xdt = _padded(x3.reshape(1, B * Ltok, 3 * D), 3), _padded(x3d.reshape(1, B * Ltok, 3 * D), 3)
    dst = torch.full((B * Ltok + 3, D), NAN, dtype=torch.bfloat16, device=dev())
    dstd = torch.full_like(dst, NAN)
    wg = w.float().to(dev())
    bad = []
    for rope in (True, False):
        _lib.check(_lib.lib().fg_op_wan_rms_rope_jvp(_p(xt, D), _p(xdt, D), 3 * D, _p(wg), 1e-6, _p(cs) if rope else None, _p(dst), _p(dstd),
                                                     B * Ltok, Ltok, D, _stream()))
        torch.cuda.synchronize()
        assert bool(dst[B * Ltok:].isnan().all()) and bool(dstd[B * Ltok:].isnan().all())

        def ref(**kw):
            n, nd = J.rms_jvp(x, xd, w, 1e-6, **kw)
            if rope:
                n, nd = (J.rope(a.view(B, Ltok, H, 128), cos, sin).flatten(2) for a in (n, nd))
            return n, nd

        want, wantd = ref()
        got, gotd = (t[:B * Ltok].double().cpu().view(B, Ltok, D) for t in (dst, dstd))
        tag = f"rms_rope {grid} D{D} {'rope' if rope else 'plain'}"
        _hold(tag + " n", got, want, (2,), OP_TOL["rms"], bad)
        _hold(tag + " nd", gotd, wantd, (2,), OP_TOL["rms_d"], bad)
        _mutant(tag + " drop_proj", gotd, ref(drop_proj=True)[1], OP_TOL["rms_d"], bad)
    assert not bad, bad


@pytest.mark.parametrize("grid", list(GRIDS))
def test_gelu_jvp(grid):
    B, Fr, gh, gw = GRIDS[grid]
    M, K = B * Fr * gh * gw, 512
    h, hd = _tokens(1, M, K, 31)
    h = J.bf16_exact(h - 0.3)
    ht, hdt = _padded(h, 3), _padded(hd, 3)
    a = torch.full_like(ht, NAN)
    ad = torch.full_like(ht, NAN)
    _lib.check(_lib.lib().fg_op_wan_gelu_jvp(_p(ht), _p(hdt), _p(a), _p(ad), M * K, _stream()))
    torch.cuda.synchronize()
    assert bool(a[:, M:].isnan().all()) and bool(ad[:, M:].isnan().all())
    want, wantd = J.gelu_jvp(h, hd)
    bad = []
    _hold(f"gelu {grid} a", a[:, :M].double().cpu(), want, (2,), OP_TOL["gelu"], bad)
    _hold(f"gelu {grid} ad", ad[:, :M].double().cpu(), wantd, (2,), OP_TOL["gelu_d"], bad)
    # in place, as the engine runs it
    _lib.check(_lib.lib().fg_op_wan_gelu_jvp(_p(ht), _p(hdt), _p(ht), _p(hdt), M * K, _stream()))
    assert torch.equal(ht[:, :M], a[:, :M]) and torch.equal(hdt[:, :M], ad[:, :M])
    assert not bad, bad


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_final_jvp(grid, D):
    B, Fr, gh, gw = GRIDS[grid]
    Ltok, C = Fr * gh * gw, 16
    x, xd = _tokens(B, Ltok, D, 41 + D)
    so, sod = _mod_rows(B, Fr, 2, D, 42 + D)
    g = torch.Generator().manual_seed(43)
    p = {"proj_out.weight": (torch.randn(4 * C, D, generator=g) * D ** -0.5).double(), "proj_out.bias": (0.05 * torch.randn(4 * C, generator=g)).double()}
    cfg = types.SimpleNamespace(eps=1e-6)
    xt, xdt = _padded(x.reshape(1, B * Ltok, D), 3), _padded(xd.reshape(1, B * Ltok, D), 3)
    out = torch.full((B, C, Fr, 2 * gh, 2 * gw), NAN, device=dev())
    outd = torch.full_like(out, NAN)
    f32 = lambda t: t.float().to(dev()).contiguous()  # noqa: E731
    mg, mdg, wg, bg = f32(so), f32(sod), f32(p["proj_out.weight"]), f32(p["proj_out.bias"])
    _lib.check(_lib.lib().fg_op_wan_final_jvp(_p(xt), _p(xdt), _p(mg), _p(mdg), _p(wg), _p(bg), _p(out), _p(outd), B, C, Fr, gh, gw, D, 1e-6, _stream()))
    torch.cuda.synchronize()
    want, wantd = J.final_jvp(p, cfg, x, xd, so, sod, Fr, gh, gw)
    bad = []
    dims = (1, 2, 3, 4)
    _hold(f"final {grid} D{D} out", out.double().cpu(), want, dims, OP_TOL["final"], bad)
    _hold(f"final {grid} D{D} jvp", outd.double().cpu(), wantd, dims, OP_TOL["final_d"], bad)
    _mutant(f"final {grid} D{D} drop_mod", outd.double().cpu(), J.final_jvp(p, cfg, x, xd, so, sod, Fr, gh, gw, drop_mod=True)[1], OP_TOL["final_d"], bad)
    assert not bad, bad
