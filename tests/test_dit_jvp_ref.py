"""CPU tests of the DiT forward-mode derivative: (1) every function of tests/dit_jvp_ref.py (the fp64 mirror of
fastgen_amd/csrc/dit_jvp.hip) against `torch.func.jvp` of the corresponding oracle function (oracle/dit_ref.py) and against a central
difference; (2) the host API of `fg_dit_jvp` / `DiT.jvp`: symbols, workspace sizes, refusals - none of which needs a device."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import dit_jvp_ref as J
from fastgen_amd import _lib
from oracle import dit_ref as R

F64 = torch.float64
# fp64 against torch.func.jvp: rounding only.  Central difference with step H: truncation H^2 |f'''| / 6 + rounding eps |f| / H
# ~ 1e-12 + 2e-10 relative for O(1) functions; the time direction under scale_t has derivatives 1000 times larger (the Fourier
# features oscillate in 1000 t), so its step is 1e-9 in t.
TOL_JVP, TOL_FD, H = 1e-11, 2e-6, 1e-6


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def _pin(fn, primals, tangents, got, h=H, tol_fd=TOL_FD):
    """got = (value, tangent) of the mirror; fn the oracle function."""
    want = torch.func.jvp(fn, primals, tangents)
    assert _rel(got[0], want[0]) < TOL_JVP and _rel(got[1], want[1]) < TOL_JVP, (_rel(got[0], want[0]), _rel(got[1], want[1]))
    plus = fn(*[p + h * v for p, v in zip(primals, tangents)])
    minus = fn(*[p - h * v for p, v in zip(primals, tangents)])
    fd = (plus - minus) / (2 * h)
    assert _rel(got[1], fd) < tol_fd, _rel(got[1], fd)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_fourier_features():
    g = _g(1)
    t, td = 1000 * torch.rand(5, generator=g, dtype=F64), torch.randn(5, generator=g, dtype=F64)
    _pin(R.fourier_features, (t,), (td,), J.fourier_jvp(t, td), h=1e-5)


def test_layer_norm_modulate():
    g = _g(2)
    x, xd = (torch.randn(2, 7, 384, generator=g, dtype=F64) for _ in range(2))
    sh, shd, sc, scd = (torch.randn(2, 384, generator=g, dtype=F64) for _ in range(4))
    fn = lambda a, b, c: R.modulate(R.layer_norm(a), b, c)  # noqa: E731
    _pin(fn, (x, sh, sc), (xd, shd, scd), J.ln_modulate_jvp(x, xd, sh, shd, sc, scd))
    # the switch drops exactly the n sd + bd terms
    n = R.layer_norm(x)
    full, cut = J.ln_modulate_jvp(x, xd, sh, shd, sc, scd)[1], J.ln_modulate_jvp(x, xd, sh, shd, sc, scd, drop_mod_tangent=True)[1]
    assert _rel(full - cut, n * scd.unsqueeze(1) + shd.unsqueeze(1)) < 1e-12


@pytest.mark.parametrize("heads,hd", [(3, 64), (2, 72)])
def test_attention(heads, hd):
    """The whole oracle `attention` (qkv, core, proj): pins the core's formula through the oracle's own head split."""
    g = _g(3)
    D = heads * hd
    cfg = R.DiTConfig(hidden_size=D, depth=1, num_heads=heads)
    sd = {k: v.double() for k, v in R.random_state_dict(cfg, seed=5).items()}
    x, xd = (torch.randn(2, 40, D, generator=g, dtype=F64) for _ in range(2))
    _pin(lambda a: R.attention(sd, "blocks.0.", a, heads), (x,), (xd,), J.attention_jvp(sd, "blocks.0.", x, xd, heads))
    q, k, v, qd, kd, vd = (torch.randn(2, heads, 40, hd, generator=g, dtype=F64) for _ in range(6))
    core = lambda a, b, c: ((a * hd ** -0.5) @ b.transpose(-2, -1)).softmax(dim=-1) @ c  # noqa: E731  (oracle `attention`, its core lines)
    _pin(core, (q, k, v), (qd, kd, vd), J.attention_core_jvp(q, k, v, qd, kd, vd))
    p = ((q * hd ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
    assert _rel(J.attention_core_jvp(q, k, v, qd, kd, vd, drop_softmax_term=True)[1], p @ vd) < 1e-12


def test_gelu_tanh():
    h = torch.linspace(-6, 6, 4001, dtype=F64)
    hd = torch.randn(4001, generator=_g(4), dtype=F64)
    _pin(lambda a: F.gelu(a, approximate="tanh"), (h,), (hd,), J.gelu_jvp(h, hd))


def test_time_embedding_and_silu():
    cfg = R.DiTConfig(hidden_size=384, depth=1, num_heads=6)
    sd = {k: v.double() for k, v in R.random_state_dict(cfg, seed=6).items()}
    g = _g(5)
    t, td = 1000 * torch.rand(4, generator=g, dtype=F64), torch.randn(4, generator=g, dtype=F64)
    _pin(lambda a: R.time_embedding(sd, "t_embedder", a), (t,), (td,), J.time_embedding_jvp(sd, "t_embedder", t, td), h=1e-5)
    v, vd = (torch.randn(50, generator=g, dtype=F64) * 3 for _ in range(2))
    _pin(F.silu, (v,), (vd,), J.silu_jvp(v, vd))


def test_dit_block():
    cfg = R.DiTConfig(hidden_size=384, depth=2, num_heads=6)
    sd = {k: v.double() for k, v in R.random_state_dict(cfg, seed=7).items()}
    g = _g(6)
    x, xd = (torch.randn(2, 48, 384, generator=g, dtype=F64) for _ in range(2))
    c, cd = (torch.randn(2, 384, generator=g, dtype=F64) for _ in range(2))
    _pin(lambda a, b: R.dit_block(sd, 1, a, b, 6), (x, c), (xd, cd), J.dit_block_jvp(sd, 1, x, xd, c, cd, 6))
    full = J.dit_block_jvp(sd, 1, x, xd, c, cd, 6)[1]
    for sw in ("drop_softmax_term", "drop_gate_tangent", "drop_mod_tangent"):
        assert _rel(J.dit_block_jvp(sd, 1, x, xd, c, cd, 6, **{sw: True})[1], full) > 1e-2, sw


@pytest.mark.parametrize("kw", [dict(r_timestep=True, time_cond_type="diff", scale_t=False), dict(r_timestep=True, scale_t=True),
                                dict(use_sit_convention=True)], ids=["r-diff", "r-abs-scale_t", "sit"])
def test_whole_network(kw):
    """dit_jvp (preparation of t / r and its chain rule included) against torch.func.jvp over the oracle's dit_forward."""
    cfg = R.DiTConfig(hidden_size=384, depth=2, num_heads=6, **kw)
    sd = {k: v.double() for k, v in R.random_state_dict(cfg, seed=77).items()}
    g = _g(8)
    x, vx = (torch.randn(2, 4, 32, 32, generator=g, dtype=F64) for _ in range(2))
    t = 0.1 + 0.8 * torch.rand(2, generator=g, dtype=F64)
    r = t * torch.rand(2, generator=g, dtype=F64) if cfg.r_timestep else None
    vt = torch.ones(2, dtype=F64)
    vr = torch.tensor([0.5, -0.7], dtype=F64) if cfg.r_timestep else None
    cls = torch.tensor([3, 1000])
    got = J.dit_jvp(sd, cfg, x, t, cls, r, vx, vt, vr)
    want = J.oracle_jvp(sd, cfg, x, t, cls, r, vx, vt, vr)
    assert _rel(got[0], want[0]) < TOL_JVP and _rel(got[1], want[1]) < TOL_JVP, (_rel(got[0], want[0]), _rel(got[1], want[1]))
    h = 1e-9 if cfg.scale_t else 1e-6
    f = lambda s: R.dit_forward(sd, cfg, x + s * vx, t + s * vt, cls, None if r is None else r + s * vr)  # noqa: E731
    fd = (f(h) - f(-h)) / (2 * h)
    assert _rel(got[1], fd) < (2e-4 if cfg.scale_t else TOL_FD), _rel(got[1], fd)  # (step 1e-9: rounding eps / h = 2e-7 per unit of |f| / |f'|)
    if cfg.time_cond_type == "diff":
        assert _rel(J.dit_jvp(sd, cfg, x, t, cls, r, vx, vt, vr, flip_vr=True)[1], got[1]) > 1e-2


# ---- host API (fails without fg_dit_jvp) ---------------------------------------------------------------------------------------------
def _handle(dtype=_lib.FG_DTYPE_BF16X3, input_size=32, hidden=384, heads=6, r=1):
    cfg = _lib.fg_dit_config()
    cfg.input_size, cfg.patch_size, cfg.in_channels, cfg.hidden_size, cfg.depth, cfg.num_heads = input_size, 2, 4, hidden, 2, heads
    cfg.mlp_hidden, cfg.embedding_rows, cfg.r_timestep, cfg.compute_dtype = 4 * hidden, 1001, r, dtype
    h = ctypes.c_void_p()
    _lib.check(_lib.lib().fg_dit_create(ctypes.byref(cfg), ctypes.byref(h)))
    return h


def test_symbols_resolve():
    L = _lib.lib()
    for name in ("fg_dit_jvp", "fg_dit_jvp_workspace_bytes", "fg_op_dit_ln_modulate_jvp", "fg_op_dit_attention_jvp", "fg_op_dit_gelu_jvp"):
        assert getattr(L, name) is not None and name in _lib.SIGNATURES


def test_workspace_bytes():
    L = _lib.lib()
    for hidden, heads in ((384, 6), (1152, 16)):
        h = _handle(hidden=hidden, heads=heads)
        try:
            for B in (1, 3, 64):
                assert L.fg_dit_jvp_workspace_bytes(h, B) > L.fg_dit_workspace_bytes(h, B) > 0
                assert L.fg_dit_jvp_workspace_bytes(h, B) % 256 == 0
            assert L.fg_dit_jvp_workspace_bytes(h, 0) == 0 and L.fg_dit_jvp_workspace_bytes(None, 1) == 0
        finally:
            L.fg_dit_destroy(h)
    for kw in (dict(dtype=_lib.FG_DTYPE_F32), dict(dtype=_lib.FG_DTYPE_BF16), dict(dtype=_lib.FG_DTYPE_FP8), dict(input_size=64)):
        h = _handle(**kw)
        try:
            assert L.fg_dit_workspace_bytes(h, 2) > 0 and L.fg_dit_jvp_workspace_bytes(h, 2) == 0, kw
        finally:
            L.fg_dit_destroy(h)


def test_jvp_refuses_bad_arguments_without_a_device():
    L = _lib.lib()
    h = _handle()
    # made-up, well separated addresses: they stand for every pointer (nothing is read before the checks are through)
    one, two, three, ws = (ctypes.c_void_p(a << 28) for a in (1, 2, 3, 4))
    base = 4 << 28
    good = [h, one, one, one, one, one, one, one, two, three, 1, ws, 256, None]
    try:
        assert L.fg_dit_jvp(*good) == 2 and b"not packed" in L.fg_last_error()  # FG_ENOTREADY: every argument check is through
        for i in (0, 1, 2, 4, 5, 8, 9, 11):  # h, x_t, t, class_ids, vx, out, jvp, workspace (r, vt, vr are nullable)
            a = list(good)
            a[i] = None
            assert L.fg_dit_jvp(*a) == 1, i
            assert b"fg_dit_jvp" in L.fg_last_error()
        for i in (3, 6, 7):
            a = list(good)
            a[i] = None
            assert L.fg_dit_jvp(*a) == 2, i
        for batch in (0, -1, 1 << 23):
            a = list(good)
            a[10] = batch
            assert L.fg_dit_jvp(*a) == 1 and b"batch" in L.fg_last_error()
        a = list(good)
        a[11] = ctypes.c_void_p(base + 128)
        assert L.fg_dit_jvp(*a) == 1 and b"256-byte aligned" in L.fg_last_error()
        for i, j in ((8, 1), (9, 5), (9, 8)):  # out = x_t, jvp = vx, jvp = out
            a = list(good)
            a[i] = a[j]
            assert L.fg_dit_jvp(*a) == 1 and b"alias" in L.fg_last_error(), (i, j)
    finally:
        L.fg_dit_destroy(h)
    for kw in (dict(dtype=_lib.FG_DTYPE_F32), dict(dtype=_lib.FG_DTYPE_BF16), dict(dtype=_lib.FG_DTYPE_FP8), dict(input_size=64)):
        h = _handle(**kw)
        try:
            assert L.fg_dit_jvp(*([h] + good[1:])) == 1 and b"bf16x3 compute mode on a 16 x 16 token grid" in L.fg_last_error(), kw
        finally:
            L.fg_dit_destroy(h)


def test_ops_refuse_bad_arguments_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 255) & ~255
    p = [ctypes.c_void_p(base + 256 * i) for i in range(8)]
    ln = lambda **kw: L.fg_op_dit_ln_modulate_jvp(*{**dict(x=p[0], xd=p[1], mod=p[2], modd=p[3], ms=2304, so=0, co=384, y=p[4], yd=p[5], ntok=512,  # noqa: E731
                                                          d=384, tpi=256, s=None), **kw}.values())
    for kw in (dict(x=None), dict(modd=None), dict(yd=None), dict(d=512), dict(ntok=0), dict(tpi=0), dict(ms=2305), dict(so=1), dict(co=2000),
               dict(yd=p[4]), dict(y=p[0]), dict(x=ctypes.c_void_p(base + 4))):
        assert ln(**kw) == 1 and b"fg_op_dit_ln_modulate_jvp" in L.fg_last_error(), kw
    lo = 2 * 3 * 256 * 64 + 32 * 256
    at = lambda **kw: L.fg_op_dit_attention_jvp(*{**dict(q=p[0], k=p[1], vt=p[2], qd=p[3], kd=p[4], vtd=p[5], out=p[6], outd=p[7], b=2, heads=3,  # noqa: E731
                                                        hd=64, T=256, lo=lo, s=None), **kw}.values())
    for kw in (dict(q=None), dict(vtd=None), dict(outd=None), dict(b=0), dict(heads=0), dict(hd=128), dict(T=1024), dict(T=128), dict(lo=lo - 8),
               dict(lo=lo + 4), dict(outd=p[6]), dict(k=ctypes.c_void_p(base + 8))):
        assert at(**kw) == 1 and b"fg_op_dit_attention_jvp" in L.fg_last_error(), kw
    ge = lambda **kw: L.fg_op_dit_gelu_jvp(*{**dict(h=p[0], hd=p[1], a=p[2], ad=p[3], m=512, k=1536, s=None), **kw}.values())  # noqa: E731
    for kw in (dict(h=None), dict(ad=None), dict(m=0), dict(k=0), dict(k=1538), dict(ad=p[2]), dict(a=p[1]), dict(hd=ctypes.c_void_p(base + 4))):
        assert ge(**kw) == 1 and b"fg_op_dit_gelu_jvp" in L.fg_last_error(), kw


def test_module_refusals():
    from fastgen_amd.methods.consistency_model.mean_flow import MeanFlowModel
    from fastgen_amd.networks.DiT.network import DiT

    kw = dict(hidden_size=384, depth=1, num_heads=6)
    x, t = torch.zeros(1, 4, 32, 32), torch.full((1,), 0.5)
    cond = torch.tensor([1])
    with pytest.raises(NotImplementedError, match="bf16x3"):
        DiT(compute_dtype="bf16", **kw).jvp(x, t, x, condition=cond)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        DiT(compute_dtype="fp8", **kw).jvp(x, t, x, condition=cond)
    x64 = torch.zeros(1, 4, 64, 64)
    with pytest.raises(NotImplementedError, match="16 x 16 token grid"):
        DiT(input_size=64, **kw).jvp(x64, t, x64, condition=cond)
    net = DiT(compute_dtype="bf16x3", **kw)
    with pytest.raises(RuntimeError, match="HIP GPU only"):
        net.jvp(x, t, x, condition=cond)
    with pytest.raises(NotImplementedError, match="own prediction type"):
        net.jvp(x, t, x, condition=cond, fwd_pred_type="x0")
    netr = DiT(compute_dtype="bf16x3", r_timestep=True, **kw)
    with pytest.raises(ValueError, match="needs r"):
        netr.jvp(x, t, x, condition=cond)
    with pytest.raises(RuntimeError, match="HIP GPU only"):  # (a DiT has a jvp: network_jvp reaches it)
        MeanFlowModel.network_jvp(netr, x, t, 0.5 * t, x, condition=cond)
