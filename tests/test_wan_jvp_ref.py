"""CPU checks of tests/wan_jvp_ref.py, the fp64 mirror of the bidirectional video DiT's forward-mode derivative (`fg_wan_jvp`): (1) every
function against `torch.func.jvp` of the corresponding piece of oracle/wan_ref.py (to ~1e-10) and against a central difference; (2) the
tile-by-tile restatement of the attention kernel's algorithm against the direct formula, for c_i = 0, the first-tile mean and an
arbitrary c_i, with a ragged last tile; (3) the hand-carried whole-network tangent `net_jvp` against `torch.func.jvp` over
`forward_rows`, and that against `torch.func.jvp` over tests/wan_full_ref.py's `WanFullRef.forward` in (x, t, r); (4) how far every mutant
stands from the reference at the seeds and shapes of the GPU tests, as a multiple of their bounds; (5) the host API: symbols, workspace
queries, refusals and `Wan.jvp`'s errors - none of which needs a device."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import wan_full_ref as W
import wan_jvp_ref as J
from fastgen_amd import _lib
from oracle import wan_ref as R

torch.set_default_dtype(torch.float32)
TIGHT = 1e-10


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _rand(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _fd(f, args, tans, eps=1e-6):
    """Central difference of f along tans."""
    up = f(*[a + eps * t for a, t in zip(args, tans)])
    dn = f(*[a - eps * t for a, t in zip(args, tans)])
    return (up - dn) / (2 * eps)


def _check(mine, f, args, tans, fd_tol=1e-6):
    """mine = (primal, tangent) against torch.func.jvp(f) and the central difference of f."""
    want, wantd = torch.func.jvp(f, tuple(args), tuple(tans))
    assert _rel(mine[0], want) < TIGHT and _rel(mine[1], wantd) < TIGHT, (_rel(mine[0], want), _rel(mine[1], wantd))
    assert _rel(mine[1], _fd(f, args, tans)) < fd_tol, _rel(mine[1], _fd(f, args, tans))


def _tiny(r=True, seed=3):
    cfg = R.TINY
    sd = W.random_state_dict(cfg, seed, r_timestep=r)
    return cfg, J.params64(sd), sd


# ---- (1) the formulas ------------------------------------------------------------------------------------------------------------------
def test_time_conditioning():
    cfg, p, _ = _tiny()
    t, td = 1000 * torch.rand(6, dtype=torch.float64, generator=torch.Generator().manual_seed(1)), _rand(6, seed=2, scale=1000.0)
    f, fd = J.fourier_jvp(t, td, cfg.freq_dim)
    _check((f, fd), lambda a: R.timesteps_proj(a, cfg.freq_dim), [t], [td], fd_tol=1e-5)
    e, ed, pj, pjd = J.embedder_jvp(p, cfg, t, td)
    _check((e, ed), lambda a: R.time_embedding(p, cfg, a), [t], [td], fd_tol=1e-5)
    assert _rel(J.time_embedding(p, cfg, t), R.time_embedding(p, cfg, t)) < 1e-14
    _check((pj, pjd), lambda a: R.time_projection(p, R.time_embedding(p, cfg, a)), [t], [td], fd_tol=1e-5)
    pr = J._r_params(p)
    e, ed, pj, pjd = J.embedder_jvp(pr, cfg, t, td)
    _check((pj, pjd), lambda a: R.time_projection(pr, R.time_embedding(pr, cfg, a)), [t], [td], fd_tol=1e-5)


def test_ln_modulate():
    B, Fr, fs, D = 2, 3, 5, 256
    x, xd = _rand(B, Fr * fs, D, seed=1, scale=2.0) + 0.3, _rand(B, Fr * fs, D, seed=2)
    s, b, sd, bd = (_rand(B, Fr, D, seed=3 + i, scale=0.5) for i in range(4))
    L = Fr * fs
    mine = J.ln_modulate_jvp(x, xd, J.per_frame_rows(s, L), J.per_frame_rows(b, L), J.per_frame_rows(sd, L), J.per_frame_rows(bd, L), 1e-6)
    _check(mine, lambda a, c, d: R.per_frame(R.layer_norm(a, 1e-6), c, d), [x, s, b], [xd, sd, bd])
    # the cross-attention norm: a constant affine
    w, bb = 1 + _rand(D, seed=9, scale=0.1), _rand(D, seed=10, scale=0.1)
    zero = torch.zeros((), dtype=torch.float64)
    _check(J.ln_modulate_jvp(x, xd, w - 1, bb, zero, zero, 1e-6), lambda a: R.layer_norm(a, 1e-6, w, bb), [x], [xd])
    # mutant (d) is another function
    assert _rel(J.ln_modulate_jvp(x, xd, J.per_frame_rows(s, L), J.per_frame_rows(b, L), J.per_frame_rows(sd, L), J.per_frame_rows(bd, L), 1e-6,
                                  drop_mod=True)[1], mine[1]) > 0.1


def test_rms_rope():
    cfg = R.TINY
    B, Fr, gh, gw = 2, 3, 5, 3
    L, D = Fr * gh * gw, cfg.dim
    x, xd, w = _rand(B, L, D, seed=1, scale=1.5), _rand(B, L, D, seed=2), 1 + _rand(D, seed=3, scale=0.2)
    cos, sin = R.rope_for_chunk(cfg, Fr, gh, gw, 0, torch.float64)
    hv = lambda a: a.view(B, L, cfg.num_heads, -1)  # noqa: E731
    n, nd = J.rms_jvp(x, xd, w, cfg.eps)
    _check((n, nd), lambda a: R.rms_norm(a, w, cfg.eps), [x], [xd])
    _check((J.rope(hv(n), cos, sin), J.rope(hv(nd), cos, sin)), lambda a: R.apply_rope(hv(R.rms_norm(a, w, cfg.eps)).clone(), cos, sin), [x], [xd])
    assert _rel(J.rope(hv(n), cos, sin), R.apply_rope(hv(n), cos, sin)) < 1e-15
    assert _rel(J.rms_jvp(x, xd, w, cfg.eps, drop_proj=True)[1], nd) > 0.05


def _attn_inputs(B, Lq, Lk, H=2, hd=128, seed=0, gain=3.0):
    g = lambda i, *s: _rand(*s, seed=seed + i)  # noqa: E731
    return (gain * g(0, B, Lq, H, hd) / math.sqrt(hd) ** 0.5, g(1, B, Lk, H, hd), g(2, B, Lk, H, hd), g(3, B, Lq, H, hd), g(4, B, Lk, H, hd),
            g(5, B, Lk, H, hd))


def test_attention_formula():
    q, k, v, qd, kd, vd = _attn_inputs(2, 21, 37)
    _check(J.attention_jvp(q, k, v, qd, kd, vd), J.sdpa_plain, [q, k, v], [qd, kd, vd])
    assert _rel(J.sdpa_plain(q, k, v), R.sdpa(q, k, v)) < 1e-13
    # cross-attention: the keys carry no tangent
    _check(J.attention_jvp(q, k, v, qd, None, None), lambda a: J.sdpa_plain(a, k, v), [q], [qd])
    full = J.attention_jvp(q, k, v, qd, kd, vd)[1]
    assert _rel(J.attention_jvp(q, k, v, qd, kd, vd, drop_delta=True)[1], full) > 0.1
    assert _rel(J.attention_jvp(q, k, v, qd, kd, vd, drop_pvd=True)[1], full) > 0.1


@pytest.mark.parametrize("Lk", [9, 32, 105, 137])
def test_attention_tiled_equals_direct(Lk):
    """(2): online rescale, c_i from the first tile, 32-key tiles, a ragged last tile - exact for every c_i."""
    q, k, v, qd, kd, vd = _attn_inputs(2, 40, Lk, seed=10)
    kd = kd + 50.0 * _rand(1, 1, 2, 128, seed=77)  # a row common to all keys, far larger than the rest (the shift tangent)
    want = J.attention_jvp(q, k, v, qd, kd, vd)
    arb = _rand(2, 2, 40, seed=5, scale=30.0)
    for c in (0.0, "mean", arb):
        got = J.attention_jvp_tiled(q, k, v, qd, kd, vd, c=c)
        assert _rel(got[0], want[0]) < 1e-13 and _rel(got[1], want[1]) < 1e-9, (c if not torch.is_tensor(c) else "arb", _rel(got[1], want[1]))
    got = J.attention_jvp_tiled(q, k, v, qd, None, None, c="mean")
    want = J.attention_jvp(q, k, v, qd, None, None)
    assert _rel(got[1], want[1]) < 1e-12


def test_gated_residual_and_gelu():
    B, L, D, K = 2, 15, 64, 96
    x, xd, o, od = _rand(B, L, D, seed=1), _rand(B, L, D, seed=2), _rand(B, L, K, seed=3), _rand(B, L, K, seed=4)
    Wm, b, g, gd = _rand(D, K, seed=5, scale=K ** -0.5), _rand(D, seed=6), _rand(B, L, D, seed=7), _rand(B, L, D, seed=8)
    mine = J.gated_residual_jvp(x, xd, o, od, Wm, b, g, gd)
    _check(mine, lambda a, c, e: a + e * F.linear(c, Wm, b), [x, o, g], [xd, od, gd])
    _check(J.gated_residual_jvp(x, xd, o, od, Wm, b), lambda a, c: a + F.linear(c, Wm, b), [x, o], [xd, od])
    assert _rel(J.gated_residual_jvp(x, xd, o, od, Wm, b, g, gd, drop_gate=True)[1], mine[1]) > 0.1
    h, hd = _rand(B, L, K, seed=9, scale=2.0), _rand(B, L, K, seed=10)
    _check(J.gelu_jvp(h, hd), lambda a: F.gelu(a, approximate="tanh"), [h], [hd])


def test_patch_embed_and_final():
    cfg, p, _ = _tiny()
    B, Fr, gh, gw = 2, 3, 5, 3
    x, vx = _rand(B, 16, Fr, 2 * gh, 2 * gw, seed=1), _rand(B, 16, Fr, 2 * gh, 2 * gw, seed=2)
    _, want = torch.func.jvp(lambda a: R.patch_embed(p, a), (x,), (vx,))
    got = F.conv3d(vx, p["patch_embedding.weight"], None, stride=(1, 2, 2)).flatten(2).transpose(1, 2)
    assert _rel(got, want) < TIGHT
    L, D = Fr * gh * gw, cfg.dim
    hs, hd, temb, tembd = _rand(B, L, D, seed=3), _rand(B, L, D, seed=4), _rand(B * Fr, D, seed=5), _rand(B * Fr, D, seed=6)
    so = p["scale_shift_table"].view(1, 1, 2, D) + temb.view(B, Fr, 1, D)
    mine = J.final_jvp(p, cfg, hs, hd, so, tembd.view(B, Fr, 1, D).expand(B, Fr, 2, D), Fr, gh, gw)
    _check(mine, lambda a, e: R.final_layer(p, cfg, a, e, Fr, gh, gw), [hs, temb], [hd, tembd])


# ---- (3) the network --------------------------------------------------------------------------------------------------------------------
def _net_inputs(cfg, B, Fr, lat, seed, with_r=True, text_len=24):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cfg.in_channels, Fr, *lat, generator=g).double()
    vx = torch.randn(B, cfg.in_channels, Fr, *lat, generator=g).double()
    text = torch.randn(B, text_len, cfg.text_dim, generator=g).double()
    return (x, *J.frame_rows(B, Fr, seed + 1, with_r), text, vx)


@pytest.mark.parametrize("cond", ["diff", "abs", None])
def test_network_tangent(cond):
    cfg, p, sd = _tiny(r=cond is not None)
    x, ts, rs, vts, vrs, text, vx = _net_inputs(cfg, 2, 3, (10, 6), 11, with_r=cond is not None)
    diff = cond == "diff"
    out, jv = J.net_jvp(p, cfg, x, ts, rs, text, vx, vts, vrs, diff)
    want, wantd = J.oracle_jvp(p, cfg, x, ts, rs, text, vx, vts, vrs, diff)
    assert _rel(out, want) < TIGHT and _rel(jv, wantd) < TIGHT, (_rel(out, want), _rel(jv, wantd))
    # a central difference of the composition of the oracle's own pieces (a step of 1e-4 embedder units: 1e-7 in t)
    f = lambda a, b, c=None: J.forward_rows(p, cfg, a, b, c, text, diff)  # noqa: E731
    args, tans = ([x, ts], [vx, vts]) if rs is None else ([x, ts, rs], [vx, vts, vrs])
    assert _rel(jv, _fd(f, args, tans, eps=1e-7)) < 1e-5
    # ... and the composition is WanFullRef.forward once a sample's rows are all 1000 t / 1000 r: torch.func.jvp over it in (x, t, r),
    # whose fp32 preparation of (t, r) bounds the agreement at fp32's 1e-7
    t1, r1 = torch.tensor([0.8, 0.45], dtype=torch.float64), torch.tensor([0.3, 0.1], dtype=torch.float64)
    net = W.WanFullRef(sd, cfg, dtype=torch.float64, time_cond_type=cond or "diff")
    ex = lambda v: (1000.0 * v.float()).double().view(2, 1).expand(2, 3).contiguous()  # noqa: E731
    vt1, vr1 = torch.ones(2, dtype=torch.float64), torch.tensor([0.5, -0.25], dtype=torch.float64)
    with torch.nn.attention.sdpa_kernel(torch.nn.attention.SDPBackend.MATH):  # (the fused CPU kernel has no forward-mode rule)
        if cond is None:
            w0, w1 = torch.func.jvp(lambda a, b: net.forward(a, b, text), (x, t1), (vx, vt1))
            g0, g1 = J.net_jvp(p, cfg, x, ex(t1), None, text, vx, ex(vt1), None, diff)
        else:
            w0, w1 = torch.func.jvp(lambda a, b, c: net.forward(a, b, text, r=c), (x, t1, r1), (vx, vt1, vr1))
            g0, g1 = J.net_jvp(p, cfg, x, ex(t1), ex(r1), text, vx, ex(vt1), ex(vr1), diff)
    assert _rel(g0, w0) < 1e-6 and _rel(g1, w1) < 1e-5, (_rel(g0, w0), _rel(g1, w1))


# ---- (4) the mutants at the GPU tests' seeds and shapes ---------------------------------------------------------------------------------
def test_network_mutants_stand_apart():
    """Per sample, the relative L2 distance of every mutant's tangent from the reference's in the direction (v_x, v_t, v_r) of
    tests/test_gpu_wan_jvp.py, at its two smallest cases: each must stand MUTANT_FACTOR times the network bound away in its closest
    sample (those that do not under bf16 are named in J.NET_WEAK_MUTANTS and left to the per-op file)."""
    bad = []
    for name in ("F105", "F480-diff"):
        c = J.NET_CASES[name]
        cfg, p, x, ts, rs, vts, vrs, text, vx = J.net_case(name)
        ref = J.net_jvp(p, cfg, x, ts, rs, text, vx, vts, vrs, c["r"] == "diff")[1]
        for m in J.MUTANTS:
            d = J.rel_l2(J.mutant_jvp(m, p, cfg, x, ts, rs, text, vx, vts, vrs, c["r"] == "diff"), ref)
            print(f"[wan-jvp-ref] {name} {m}: closest sample {float(d.min()):.3e} = {float(d.min()) / J.NET_TOL[0]:.1f} x bound")
            if m not in J.NET_WEAK_MUTANTS and not float(d.min()) >= J.MUTANT_FACTOR * J.NET_TOL[0]:
                bad.append((name, m, d))
    assert not bad, bad


def test_common_shift_ratio():
    """What sets J.COMMON_SHIFT: in the time direction (0, v_t, v_r) of case F105, the part of block 0's kd that is common to the keys of
    a frame (the shift tangent, through to_k and the RMSNorm) over the rest - 1.06 in fp64; the "shift" case of the attention op takes
    twice that.  The tangent is two orders of magnitude larger than k itself (the x1000 timestep scale)."""
    cfg, p, x, ts, rs, vts, vrs, text, vx = J.net_case("F105")
    B, Fr = ts.shape
    _, _, tproj, tprojd = J.embedder_jvp(p, cfg, ts.reshape(-1), vts.reshape(-1))
    _, _, pj, pjd = J.embedder_jvp(J._r_params(p), cfg, (ts - rs).reshape(-1), (vts - vrs).reshape(-1))
    hs = R.patch_embed(p, x)
    L, D = hs.shape[1:]
    mod, modd = R.modulation(p, 0, tproj + pj, B, Fr), (tprojd + pjd).view(B, Fr, 6, D)
    row = lambda m, j: J.per_frame_rows(m[:, :, j], L)  # noqa: E731
    y, yd = J.ln_modulate_jvp(hs, torch.zeros_like(hs), row(mod, 1), row(mod, 0), row(modd, 1), row(modd, 0), cfg.eps)
    W_, b_ = p["blocks.0.attn1.to_k.weight"], p["blocks.0.attn1.to_k.bias"]
    k, kd = J.rms_jvp(F.linear(y, W_, b_), F.linear(yd, W_), p["blocks.0.attn1.norm_k.weight"], cfg.eps)
    kd = kd.view(B, Fr, L // Fr, D)
    common = kd.mean(2, keepdim=True)
    ratio = float(common.expand_as(kd).norm() / (kd - common).norm())
    print(f"[wan-jvp-ref] common / rest of kd {ratio:.3f}; |kd| / |k| {float(kd.norm() / k.norm()):.1f}")
    assert 0.5 < ratio <= J.COMMON_SHIFT


def test_attention_op_mutants_stand_apart():
    for name, c in J.ATT_CASES.items():
        if c["Lq"] > 600:
            continue  # (the long case runs on the device)
        q, k, v, qd, kd, vd = J.att_case(name)
        ref = J.attention_jvp(q, k, v, qd, kd, vd)[1]
        for m in ("drop_delta", "drop_pvd"):
            if (m == "drop_pvd" and vd is None) or name in J.ATT_MUTANT_SKIP.get(m, ()):
                continue
            mut = J.attention_jvp(q, k, v, qd, kd, vd, **{m: True})[1]
            d = J.rel_l2(mut, ref)
            print(f"[wan-jvp-ref] attention {name} {m}: closest sample {float(d.min()):.3e} = {float(d.min()) / J.ATT_TOL['od'][0]:.1f} x bound")
            assert float(d.min()) >= J.MUTANT_FACTOR * J.ATT_TOL["od"][0], (name, m, d)


# ---- (5) host API (fails without fg_wan_jvp) ---------------------------------------------------------------------------------------------
_handle = J.make_handle


def test_symbols_and_workspace_queries():
    L = _lib.lib()
    for name in ("fg_wan_jvp", "fg_wan_jvp_workspace_bytes", "fg_op_wan_attention_jvp", "fg_op_wan_modulate_jvp", "fg_op_wan_rms_rope_jvp",
                 "fg_op_wan_gelu_jvp", "fg_op_wan_final_jvp"):
        assert hasattr(L, name), name
    h = _handle()
    try:
        need = L.fg_wan_jvp_workspace_bytes(h, 2, 5, 16, 24)
        assert need > 0 and need % 256 == 0 and L.fg_wan_jvp_workspace_bytes(h, 4, 5, 16, 24) > need
        assert L.fg_wan_jvp_workspace_bytes(h, 0, 5, 16, 24) == 0 and L.fg_wan_jvp_workspace_bytes(h, 2, 5, 15, 24) == 0
        assert L.fg_wan_jvp_workspace_bytes(None, 2, 5, 16, 24) == 0
    finally:
        L.fg_wan_destroy(h)
    for kw in (dict(dtype="fp8"), dict(kind="i2v"), dict(kind="vace")):
        h = _handle(**kw)
        try:
            assert L.fg_wan_full_workspace_bytes(h, 2, 5, 16, 24) > 0 and L.fg_wan_jvp_workspace_bytes(h, 2, 5, 16, 24) == 0, kw
        finally:
            L.fg_wan_destroy(h)


def test_argument_refusals_need_no_device():
    """Every argument check of fg_wan_jvp comes before the handle's state: on an unpacked handle a good call ends at FG_ENOTREADY."""
    L = _lib.lib()
    FG_EINVAL, FG_ENOTREADY = 1, 2
    fake = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(10)]
    h = _handle()
    try:
        def call(hh=h, x=fake[0], t=fake[1], r=fake[2], vx=fake[3], vt=fake[4], vr=fake[5], out=fake[6], jv=fake[7], skip=None, nskip=0, ws=fake[8]):
            return L.fg_wan_jvp(hh, x, t, r, vx, vt, vr, out, jv, 2, 5, 16, 24, skip, nskip, ws, 1 << 40, None)
        assert call() == FG_ENOTREADY and b"not packed" in L.fg_last_error()
        assert call(r=None, vr=None, vt=None) == FG_ENOTREADY
        assert call(skip=(ctypes.c_int * 1)(0), nskip=1) == FG_EINVAL and b"skip_layers" in L.fg_last_error()
        assert call(out=fake[0]) == FG_EINVAL and b"alias" in L.fg_last_error()
        for other in (fake[0], fake[1], fake[2], fake[3], fake[4], fake[5], fake[6]):
            assert call(jv=other) == FG_EINVAL and b"alias" in L.fg_last_error()
        assert call(r=None) == FG_EINVAL and b"vr_frames" in L.fg_last_error()
        assert call(x=None) == FG_EINVAL and call(ws=ctypes.c_void_p(0x1001)) == FG_EINVAL
    finally:
        L.fg_wan_destroy(h)
    h = _handle(r=0)
    try:
        assert L.fg_wan_jvp(h, fake[0], fake[1], fake[2], fake[3], None, None, fake[6], fake[7], 2, 5, 16, 24, None, 0, fake[8], 1 << 40,
                            None) == FG_EINVAL and b"r_embedder" in L.fg_last_error()
    finally:
        L.fg_wan_destroy(h)
    for kw, msg in ((dict(dtype="fp8"), b"fp8"), (dict(kind="i2v"), b"image-to-video"), (dict(kind="vace"), b"VACE")):
        h = _handle(**kw)
        try:
            assert L.fg_wan_jvp(h, fake[0], fake[1], None, fake[3], None, None, fake[6], fake[7], 2, 5, 16, 24, None, 0, fake[8], 1 << 40,
                                None) == FG_EINVAL and msg in L.fg_last_error(), kw
        finally:
            L.fg_wan_destroy(h)
    # the handle-free ops check their arguments before they launch
    p = fake
    assert L.fg_op_wan_attention_jvp(p[0], p[1], 260, 0, p[2], p[3], None, None, 256, 0, p[4], p[5], 256, 0, 1, 2, 10, 10, None) == FG_EINVAL
    assert L.fg_op_wan_attention_jvp(p[0], p[1], 256, 0, p[2], p[3], None, None, 256, 0, p[4], p[4], 256, 0, 1, 2, 10, 10, None) == FG_EINVAL
    att = lambda **kw: L.fg_op_wan_attention_jvp(*{**dict(q=p[0], qd=p[1], ldq=256, q_bs=2560, k=p[2], v=p[3], kd=None, vd=None, ldk=256, kv_bs=2560,  # noqa: E731
                                                          out=p[4], outd=p[5], ldo=256, o_bs=2560, b=2, h=2, lq=10, lkv=10, s=None), **kw}.values())
    odd = ctypes.c_void_p(0x1008)
    for kw in (dict(q_bs=2564), dict(kv_bs=2564), dict(o_bs=2562), dict(q=odd), dict(qd=odd), dict(k=odd), dict(v=odd), dict(kd=odd), dict(vd=odd),
               dict(out=ctypes.c_void_p(0x1004)), dict(outd=ctypes.c_void_p(0x1004))):
        assert att(**kw) == FG_EINVAL and b"fg_op_wan_attention_jvp" in L.fg_last_error(), kw
    assert L.fg_op_wan_modulate_jvp(p[0], p[1], p[2], None, 0, 0, 320, p[3], p[4], 10, 320, 10, 1e-6, None) == FG_EINVAL
    assert L.fg_op_wan_rms_rope_jvp(p[0], p[1], 256, p[2], 1e-6, None, p[3], p[4], 10, 3, 256, None) == FG_EINVAL
    assert L.fg_op_wan_gelu_jvp(p[0], p[1], p[2], p[3], 6, None) == FG_EINVAL
    assert L.fg_op_wan_final_jvp(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[6], 1, 16, 1, 2, 2, 256, 1e-6, None) == FG_EINVAL


def test_module_jvp_errors_on_the_cpu():
    """`Wan.jvp` exists and refuses CPU tensors; the networks without a tangent say so (or have no `jvp`)."""
    from fastgen_amd.methods.consistency_model.mean_flow import MeanFlowModel
    from fastgen_amd.networks.Wan.network import Wan
    from fastgen_amd.networks.Wan.network_causal import CausalWan

    kw = dict(num_attention_heads=2, attention_head_dim=128, text_dim=64, ffn_dim=512, num_layers=1, rope_max_seq_len=8)
    net = Wan(r_timestep=True, **kw)
    x, t = torch.randn(1, 16, 2, 4, 4), torch.tensor([0.5])
    text = torch.randn(1, 5, 64)
    with pytest.raises(NotImplementedError, match="GPU"):
        net.jvp(x, t, torch.randn_like(x), torch.ones(1), condition=text, r=torch.tensor([0.2]))
    with pytest.raises(NotImplementedError, match="prediction type"):
        net.jvp(x, t, torch.randn_like(x), condition=text, r=torch.tensor([0.2]), fwd_pred_type="x0")
    with pytest.raises(ValueError, match="needs r"):
        net.jvp(x, t, torch.randn_like(x), condition=text)
    with pytest.raises(ValueError, match="no r_embedder"):
        Wan(r_timestep=False, **kw).jvp(x, t, torch.randn_like(x), condition=text, r=torch.tensor([0.2]))
    with pytest.raises(NotImplementedError):
        MeanFlowModel.network_jvp(net, x, t, torch.tensor([0.2]), torch.randn_like(x), condition=text)
    # the subclasses and the fp8 mode are refused on the handle's kind, before their (other) shapes are looked at
    from fastgen_amd.networks.VaceWan.network import VACEWan
    from fastgen_amd.networks.WanI2V.network import WanI2V

    small = dict(num_attention_heads=2, attention_head_dim=128, text_dim=64, ffn_dim=512, num_layers=1)
    for other in (WanI2V(image_dim=0, **small), VACEWan(vace_layers=[0], **small), Wan(compute_dtype="fp8", **small)):
        with pytest.raises(NotImplementedError, match="no forward-mode derivative"):
            other.jvp(x, t, torch.randn_like(x), condition=text)
    causal = CausalWan(chunk_size=1, total_num_frames=2, **kw)
    assert not hasattr(causal, "jvp")
    with pytest.raises(NotImplementedError, match="CausalWan"):
        MeanFlowModel.network_jvp(causal, x, t, torch.tensor([0.2]), torch.randn_like(x), condition=text)
