"""Per-op, per-block and in-situ parity of the EDM2 kernels and of the shared linear against the fp64 references of tests/edm2_ops_ref.py
and tests/edm2_ref.py run in fp64: the convolution's EDM2 fields (fg_op_adm_conv_ex), the cosine attention (fg_op_edm2_attention), the
weight preparation, the pixel norm, every dispatch arm of launch_linear (fg_op_linear), every Block through fg_edm2_run_block, every
Block's output inside a whole forward (fg_edm2_forward_taps), and three end-to-end properties: zero gains, repacking after a weight
changed, drop_precond.  tests/test_edm2_ops_ref.py shows on the CPU what each bound can see (one mutant per plausible kernel error)."""
import ctypes

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks.EDM2.network import EDM2Precond

import edm2_ops_ref as R
import edm2_ref as D

pytestmark = pytest.mark.gpu

MODES = {"bf16": _lib.FG_DTYPE_BF16, "bf16x3": _lib.FG_DTYPE_BF16X3}
TOL = {"bf16x3": dict(max_abs=5e-5, rel=2e-5), "bf16": dict(max_abs=5e-2, rel=1e-2)}  # tests/test_gpu_edm2.py's


def dev():
    return torch.device("cuda:0")


def check(got, want, mode, what):
    """tests/test_gpu_edm2.py's check, the figures printed first."""
    d = got.double() - want.double()
    err, rel = d.abs().max().item(), (d.norm() / want.double().norm().clamp_min(1e-12)).item()
    print(f"\n{what} {mode}: max_abs {err:.2e} rel L2 {rel:.2e}")
    assert torch.isfinite(got).all(), what
    assert err <= TOL[mode]["max_abs"] and rel <= TOL[mode]["rel"], f"{what}: max_abs={err:.3e} rel_l2={rel:.3e} ({mode})"


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def nan_like(*shape):
    return torch.full(shape, float("nan"), device=dev())


# ---- convolution: ab_stride, resid_scale, clip --------------------------------------------------------------------------------------
def run_conv_ex(mode, name, neutral_entry=False):
    c = R.CONV_EX_CASES[name]
    L = _lib.lib()
    x, ab, stride, off, w, resid = R.conv_ex_inputs(name)
    B, C1, C2, cout, ks, H = c["B"], c["C1"], c["C2"], c["cout"], c["ks"], c["H"]
    packed = torch.empty(L.fg_op_adm_conv_pack_bytes(mode, cout, C1 + C2, ks), dtype=torch.uint8, device=dev())
    wd = w.to(dev()).contiguous()
    _lib.check(L.fg_op_adm_conv_pack(mode, wd.data_ptr(), packed.data_ptr(), cout, C1 + C2, ks, None))
    d1 = nhwc(x[:, :C1]).to(dev())
    d2 = nhwc(x[:, C1:]).to(dev()) if C2 else None
    dab = None if ab is None else ab.to(dev()).contiguous()
    pab = None if ab is None else dab.data_ptr() + 8 * off
    dres = None if resid is None else nhwc(resid).to(dev())
    out = nan_like(B, H, H, cout)
    if neutral_entry:
        _lib.check(L.fg_op_adm_conv(mode, ks, d1.data_ptr(), C1, ptr(d2), C2, B, x.shape[2], H, c["res_mode"], pab, c["silu"], packed.data_ptr(),
                                    None, ptr(dres), c["resid_mode"] or 0, out.data_ptr(), cout, None))
    else:
        _lib.check(L.fg_op_adm_conv_ex(mode, ks, d1.data_ptr(), C1, ptr(d2), C2, B, x.shape[2], H, c["res_mode"], pab, stride, c["silu"],
                                       packed.data_ptr(), None, ptr(dres), c["resid_mode"] or 0, c["resid_scale"], c["clip"], out.data_ptr(),
                                       cout, None))
    torch.cuda.synchronize()
    return nchw(out.cpu())


@pytest.mark.parametrize("name", list(R.CONV_EX_CASES))
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_conv_ex(mode, name):
    """|d| <= test_conv's bound + 2^-22 |resid_scale resid|.  Measured on an MI355X, worst max err / bound: bf16x3 0.13 (the qkv conv), bf16 without
    prologue 0.013, bf16 with prologue 0.0004."""
    got = run_conv_ex(MODES[mode], name)
    assert torch.isfinite(got).all()
    ref, _, _ = R.conv_ex_ref(name, mode == "bf16")
    err = (got.double() - ref).abs()
    r = R.ratio(err, R.conv_ex_bound(name, mode))
    print(f"\nconv_ex {mode} {name}: max err {err.max().item():.3e}, max err/bound {r:.3f}")
    assert r <= 1.0, (mode, name, r)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_conv_ex_neutral_is_adm_conv(mode):
    """(ab_stride, resid_scale, clip) = (-1, 1.0, 0.0) is fg_op_adm_conv, bit for bit: dense ab rows, a residual, no clamp."""
    c = R.CONV_EX_CASES["dense"]
    assert (R.conv_ex_inputs("dense")[2], c["resid_scale"], c["clip"]) == (-1, 1.0, 0.0)
    a, b = run_conv_ex(MODES[mode], "dense"), run_conv_ex(MODES[mode], "dense", neutral_entry=True)
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- cosine attention ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.ATTN_KINDS)
@pytest.mark.parametrize("B,T,heads", R.ATTN_SHAPES)
def test_cosine_attention(B, T, heads, kind):
    """Against fp64: |d| <= max|v^| (4e-6 + 1e-6 max_k(|q^| . |k^|) / 8) on the normalised tensors.  The fp32 CPU oracle sits at 0.04 of
    this bound, the mutants at 7x and more.  Measured on an MI355X, worst ratio: 0.042 (T = 1024, 6 heads, aligned), so the
    constants stay as they are."""
    L = _lib.lib()
    q, k, v = R.mp_attention_inputs(B, T, heads, kind, seed=T + heads + len(kind))
    ref = R.mp_attention_ref(q.double(), k.double(), v.double())
    qkv = torch.stack([q, k, v], dim=-1).permute(0, 2, 1, 3, 4).reshape(B, T, heads * 192).contiguous().to(dev())
    out = nan_like(B, T, heads * 64)
    _lib.check(L.fg_op_edm2_attention(qkv.data_ptr(), out.data_ptr(), B, T, heads, None))
    got = out.cpu().double().reshape(B, T, heads, 64).transpose(1, 2)
    assert torch.isfinite(got).all()
    r = R.ratio((got - ref).abs(), R.mp_attention_bound(q, k, v))
    print(f"\ncosine attention B={B} T={T} heads={heads} {kind}: max err/bound {r:.3f}")
    assert r <= 1.0, r


# ---- weight preparation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.PREP_CASES))
def test_prep_weight(name):
    """|d| <= 2^-18 |ref|, the padding columns and the all-zero row exactly 0.  Measured on an MI355X, worst ratio: 0.064."""
    L = _lib.lib()
    cout, cin, cin_pad, taps, gain, e0, e1, c_split = R.PREP_CASES[name]
    w = R.prep_inputs(name)
    ref = R.prep_weight_ref(name, w.double())
    dw = w.to(dev())
    dg = None if gain is None else torch.tensor([gain], dtype=torch.float32, device=dev())
    out = nan_like(cout, cin_pad, taps)
    _lib.check(L.fg_op_edm2_prep_weight(dw.data_ptr(), out.data_ptr(), cout, cin, cin_pad, taps, ptr(dg), e0, e1, c_split, None))
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    assert (got[:, cin:] == 0).all() and (got[1] == 0).all()
    r = R.ratio((got - ref).abs(), R.PREP_REL * ref.abs())
    print(f"\nprep_weight {name}: max err/bound {r:.3f}")
    assert r <= 1.0, r


# ---- pixel norm -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,C,down", R.PIXNORM_CASES)
def test_pixel_norm(B, H, C, down):
    """|d| <= 2^-20 n^ a-, n^ the fp64 normaliser, a- the mean |x| of the window; in place without the 2x2 mean; an all-zero pixel stays
    exactly 0.  Measured on an MI355X, worst ratio: 0.31 (C = 768 with the 2x2 mean)."""
    L = _lib.lib()
    x = R.pixnorm_inputs(B, H, C, down)
    ref, nrm, abar = R.pixel_norm_ref(x.double(), down)
    dx = nhwc(x).to(dev())
    out = dx if not down else nan_like(B, H, H, C)
    _lib.check(L.fg_op_edm2_pixel_norm(dx.data_ptr(), out.data_ptr(), B, H, C, down, None))
    got = nchw(out.cpu()).double()
    assert torch.isfinite(got).all()
    if down:
        assert torch.equal(dx.cpu(), nhwc(x))
    r = R.ratio((got - ref).abs(), R.PIXNORM_REL * nrm * abar)
    print(f"\npixel_norm B={B} H={H} C={C} down={down}: max err/bound {r:.3f}")
    assert r <= 1.0, r


# ---- linear ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias,silu", [(False, 0), (True, 0), (False, 1), (True, 1)])
@pytest.mark.parametrize("arm,B,I,O", R.LINEAR_CASES)
def test_linear(arm, B, I, O, with_bias, silu):
    """Every arm of launch_linear: |d| <= in 2^-24 |x| |w|^T + 2^-23 |bias| before the SiLU (x 1.1 behind it).  Measured on an MI355X,
    worst ratio: generic 0.34, KB 16 0.077, KB 64 0.013, pair 0.007."""
    L = _lib.lib()
    assert R.linear_arm(B, I, O) == arm
    x, w, bias = R.linear_inputs(B, I, O)
    bias = bias if with_bias else None
    ref, bound = R.linear_ref(x.double(), w.double(), None if bias is None else bias.double(), silu)
    dx, dw, db = x.to(dev()), w.to(dev()), None if bias is None else bias.to(dev())
    y = nan_like(B, O)
    _lib.check(L.fg_op_linear(dx.data_ptr(), dw.data_ptr(), ptr(db), y.data_ptr(), B, I, O, silu, None))
    got = y.cpu().double()
    assert torch.isfinite(got).all()
    r = R.ratio((got - ref).abs(), bound)
    print(f"\nlinear {arm} B={B} I={I} O={O} bias={with_bias} silu={silu}: max err/bound {r:.3f}")
    assert r <= 1.0, r


def test_linear_generic_arm_takes_unaligned_pointers():
    """The FMA arm has no alignment requirement: x and w 4 bytes off a 16-byte boundary."""
    L = _lib.lib()
    B, I, O = 5, 10, 256
    x, w, _ = R.linear_inputs(B, I, O)
    bx, bw = torch.zeros(B * I + 1, device=dev()), torch.zeros(O * I + 1, device=dev())
    bx[1:], bw[1:] = x.reshape(-1).to(dev()), w.reshape(-1).to(dev())
    y = nan_like(B, O)
    assert (bx.data_ptr() + 4) % 16 == 4
    _lib.check(L.fg_op_linear(bx.data_ptr() + 4, bw.data_ptr() + 4, None, y.data_ptr(), B, I, O, 0, None))
    ref, bound = R.linear_ref(x.double(), w.double(), None, 0)
    assert R.ratio((y.cpu().double() - ref).abs(), bound) <= 1.0


# ---- the network ----------------------------------------------------------------------------------------------------------------------
def make_net(cfg, sd, **kw):
    net = EDM2Precond(**cfg.kwargs(), **kw)
    net.load_state_dict(sd, strict=True)
    return net.to(dev()).eval().requires_grad_(False)


def labels_for(cfg, B):
    return torch.nn.functional.one_hot(torch.arange(B) * 3 % cfg.label_dim, cfg.label_dim).float() if cfg.label_dim else None


def run_block(net, h, ws, index, x1, x2, emb):
    L = _lib.lib()
    cout, rout = ctypes.c_int(), ctypes.c_int()
    _lib.check(L.fg_edm2_block_info(h, index, None, None, ctypes.byref(cout), None, ctypes.byref(rout), None))
    a1, a2, e = nhwc(x1).to(dev()), None if x2 is None else nhwc(x2).to(dev()), emb.contiguous().to(dev())
    out = nan_like(x1.shape[0], rout.value, rout.value, cout.value)
    _lib.check(L.fg_edm2_run_block(h, index, a1.data_ptr(), a1.shape[-1], ptr(a2), 0 if a2 is None else a2.shape[-1], e.data_ptr(),
                                   out.data_ptr(), x1.shape[0], ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()
    return nchw(out.cpu())


def run_blocks(cfg, B, mode, seed):
    """Every block of cfg through fg_edm2_run_block against D.block in fp64: [(key, max|d| / max|ref|, rel L2)]."""
    sd = D.random_state_dict(cfg, seed=seed)
    net = make_net(cfg, sd, compute_dtype=mode)
    sd64 = R.to64(sd)
    enc, dec, _, _, _ = D.layout(cfg)
    g = R.gen(seed + 1)
    res = []
    with torch.inference_mode():
        dt, h = net._engine(dev())
        ws = net._workspace(dt, h, B, dev())
        assert _lib.lib().fg_edm2_num_blocks(h) == len(enc + dec)
        c_noise = torch.linspace(-1.2, 0.9, B, dtype=torch.float64)
        lab = labels_for(cfg, B)
        emb = D.embedding(sd64, cfg, c_noise, None if lab is None else lab.double())
        for i, b in enumerate(enc + dec):
            x1 = torch.randn(B, b.cin - b.skip_c, b.res_in, b.res_in, generator=g)
            x2 = torch.randn(B, b.skip_c, b.res_in, b.res_in, generator=g) if b.skip_c else None
            xin = x1.double() if x2 is None else D.mp_cat(x1.double(), x2.double(), cfg.concat_balance)
            ref = D.block(sd64, b, cfg, xin, emb)
            got = run_block(net, h, ws, i, x1, x2, emb.float()).double()
            assert torch.isfinite(got).all(), b.key
            d = got - ref
            res.append((b.key, (d.abs().max() / ref.abs().max()).item(), (d.norm() / ref.norm()).item()))
    del net
    torch.cuda.empty_cache()
    return res


def assert_blocks(res, mode, what, rel_l2=R.BLOCK_REL_L2):
    for key, mx, rel in res:
        print(f"\nblock {what} {mode} {key}: max|d|/max|ref| {mx:.2e} rel L2 {rel:.2e}")
    for key, mx, rel in res:
        if mode == "bf16x3":
            assert mx <= R.BLOCK_MAX_REL, (key, mx)
        else:
            assert rel <= rel_l2, (key, rel)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_blocks_narrow(mode):
    """Every NARROW block at B = 3 (192, 48 and 768 output pixels at 8x8, 16x16: partial pixel tiles), ADM's per-block bounds.
    Measured on an MI355X, worst: bf16x3 max|d| / max|ref| 6.8e-6, bf16 rel L2 2.7e-3."""
    assert_blocks(run_blocks(D.NARROW, 3, mode, seed=99), mode, "narrow")


def test_blocks_in64_s():
    """Every EDM2-S block at B = 1 in bf16x3: widths 192 .. 768, concats up to 768 + 768, 6 / 9 / 12 heads.  Measured on an MI355X,
    worst max|d| / max|ref|: 6.2e-6."""
    res = run_blocks(D.IN64_S, 1, "bf16x3", seed=98)
    assert len(res) == 36
    assert_blocks(res, "bf16x3", "in64_s")


def forward_taps(net, x, t, lab, want, with_emb=True):
    """fg_edm2_forward_taps on CPU tensors; want: tap indices to fetch.  Returns (out NCHW, emb or None, {index: NCHW tap})."""
    L = _lib.lib()
    B = x.shape[0]
    dt, h = net._engine(dev())
    ws = net._workspace(dt, h, B, dev())
    n = L.fg_edm2_num_taps(h)
    R0, C = net.img_resolution, net.img_channels
    shapes = {0: (B, R0, R0, net._cfg.model_channels * net._cfg.channel_mult[0]), n - 1: (B, R0, R0, C)}
    cout, rout = ctypes.c_int(), ctypes.c_int()
    for i in range(n - 2):
        _lib.check(L.fg_edm2_block_info(h, i, None, None, ctypes.byref(cout), None, ctypes.byref(rout), None))
        shapes[i + 1] = (B, rout.value, rout.value, cout.value)
    bufs = {i: nan_like(*shapes[i]) for i in want}
    arr = (ctypes.c_void_p * n)(*[bufs[i].data_ptr() if i in bufs else None for i in range(n)])
    dx, dtt, dl = x.to(dev()), t.to(dev()), None if lab is None else lab.to(dev())
    out = nan_like(*x.shape)
    emb = nan_like(B, net._cfg.model_channels * max(net._cfg.channel_mult[: net._cfg.num_levels])) if with_emb else None
    _lib.check(L.fg_edm2_forward_taps(h, dx.data_ptr(), dtt.data_ptr(), ptr(dl), out.data_ptr(), ptr(emb), arr if want else None, n if want else 0,
                                      B, ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()
    return out.cpu(), None if emb is None else emb.cpu(), {i: nchw(b.cpu()) for i, b in bufs.items()}


def net_inputs(cfg, B, seed):
    t = torch.exp(torch.linspace(-2.5, 3.5, B, dtype=torch.float64))
    x = torch.randn(B, cfg.img_channels, cfg.img_resolution, cfg.img_resolution, generator=R.gen(seed)) * (0.5 ** 2 + t ** 2).sqrt().float().reshape(-1, 1, 1, 1)
    return x, t, labels_for(cfg, B)


def traced_ref(sd, cfg, x, t, lab):
    trace = {}
    out = D.precond_forward(R.to64(sd), cfg, x.double(), t, None if lab is None else lab.double(), trace=trace)
    keys = ["stem"] + [b.key for b in sum(D.layout(cfg)[:2], [])] + ["F"]
    return out, trace, keys


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_forward_in_situ_narrow(mode):
    """fg_edm2_forward_taps at B = 3: every tap (stem, 22 blocks, F) against the traced fp64 U-Net, emb_out <= 2e-6, and the untapped
    call bit-equal.  bf16x3: the per-block bound 2e-5 holds in situ as it stands (measured worst max|d| / max|ref| 1.3e-5, 16x16_up).
    bf16: a tap carries the rounding of every block before it - the stem alone is at rel L2 2.2e-3, the worst tap (16x16_up) at 6.2e-3 -
    so the isolated block's 5e-3 cannot hold here; the in-situ bound is the whole forward's 1e-2 of tests/test_gpu_edm2.py, 1.6x the
    measured worst.  Measured emb_out error: 1.3e-6."""
    cfg = D.NARROW
    sd = D.random_state_dict(cfg, seed=1234)
    net = make_net(cfg, sd, compute_dtype=mode)
    x, t, lab = net_inputs(cfg, 3, 41)
    ref_out, trace, keys = traced_ref(sd, cfg, x, t, lab)
    with torch.inference_mode():
        out, emb, taps = forward_taps(net, x, t, lab, range(len(keys)))
        plain, emb2, _ = forward_taps(net, x, t, lab, [])
    assert torch.equal(out, plain) and torch.equal(emb, emb2)
    e = (emb.double() - trace["emb"]).abs().max().item()
    print(f"\nin situ {mode}: emb_out max err {e:.2e}")
    assert e <= 2e-6, e
    res = []
    for i, key in enumerate(keys):
        got, ref = taps[i].double(), trace[key]
        assert torch.isfinite(got).all(), key
        d = got - ref
        res.append((key, (d.abs().max() / ref.abs().max()).item(), (d.norm() / ref.norm()).item()))
    assert_blocks(res, mode, "in situ", rel_l2=TOL["bf16"]["rel"])
    check(out, ref_out, mode, "in situ out")


def test_forward_in_situ_narrow_b33():
    """B = 33 in bf16x3: the stacked modulation (O = 3392) takes launch_linear's two-row-tile arm.  The last block's tap, F and the
    output.  Measured on an MI355X, worst: max|d| / max|ref| 1.2e-5 (F), per-image rel L2 of the output 1.1e-5."""
    cfg = D.NARROW
    sd = D.random_state_dict(cfg, seed=1234)
    net = make_net(cfg, sd, compute_dtype="bf16x3")
    assert R.linear_arm(33, 256, sum(b.cout for b in sum(D.layout(cfg)[:2], []))) == "pair"
    x, t, lab = net_inputs(cfg, 33, 43)
    ref_out, trace, keys = traced_ref(sd, cfg, x, t, lab)
    n = len(keys)
    with torch.inference_mode():
        out, _, taps = forward_taps(net, x, t, lab, [n - 2, n - 1], with_emb=False)
    res = []
    for i in (n - 2, n - 1):
        d = taps[i].double() - trace[keys[i]]
        assert torch.isfinite(d).all()
        res.append((keys[i], (d.abs().max() / trace[keys[i]].abs().max()).item(), (d.norm() / trace[keys[i]].norm()).item()))
    assert_blocks(res, "bf16x3", "in situ B=33")
    # per image: a wrong modulation row of one image (a row tile of the linear) must not hide among the other 32
    d = (out.double() - ref_out).flatten(1)
    rel = (d.norm(dim=1) / ref_out.flatten(1).norm(dim=1)).max().item()
    print(f"in situ B=33: worst per-image rel L2 {rel:.2e}")
    assert rel <= TOL["bf16x3"]["rel"], rel


# ---- three end-to-end properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_zero_gains(mode):
    """The reference's initialisation: every emb_gain and out_gain zero.  The output is exactly c_skip x_t, and every modulation row
    is exactly {1, 0}: a block's output does not depend on the embedding, bit for bit (an all-zero embedding gives c = 0 exactly)."""
    cfg = D.NARROW
    sd = D.random_state_dict(cfg, seed=7)
    for k in sd:
        if k.endswith("emb_gain") or k.endswith("out_gain"):
            sd[k] = torch.zeros_like(sd[k])
    net = make_net(cfg, sd, compute_dtype=mode)
    x, t, lab = net_inputs(cfg, 3, 47)
    with torch.inference_mode():
        out, _, taps = forward_taps(net, x, t, lab, [len(sum(D.layout(cfg)[:2], [])) + 1], with_emb=False)
        c_skip = (0.25 / (t ** 2 + 0.25)).float().reshape(-1, 1, 1, 1)
        assert torch.equal(out, c_skip * x)
        assert (list(taps.values())[0] == 0).all()
        dt, h = net._engine(dev())
        ws = net._workspace(dt, h, 3, dev())
        enc, dec, _, _, _ = D.layout(cfg)
        E = cfg.model_channels * max(cfg.channel_mult)
        sd64 = R.to64(sd)
        for i in (1, len(enc) + 3):  # an encoder block and a decoder block with a skip
            b = (enc + dec)[i]
            g = R.gen(i)
            x1 = torch.randn(3, b.cin - b.skip_c, b.res_in, b.res_in, generator=g)
            x2 = torch.randn(3, b.skip_c, b.res_in, b.res_in, generator=g) if b.skip_c else None
            a = run_block(net, h, ws, i, x1, x2, torch.zeros(3, E))
            c = run_block(net, h, ws, i, x1, x2, 3.0 * torch.randn(3, E, generator=g))
            assert torch.equal(a, c), b.key
            xin = x1.double() if x2 is None else D.mp_cat(x1.double(), x2.double(), cfg.concat_balance)
            ref = D.block(sd64, b, cfg, xin, torch.zeros(3, E, dtype=torch.float64))
            d = a.double() - ref
            if mode == "bf16x3":
                assert (d.abs().max() / ref.abs().max()).item() <= R.BLOCK_MAX_REL
            else:
                assert (d.norm() / ref.norm()).item() <= R.BLOCK_REL_L2


def sampler_ref(sd64, cfg, noise, lab, tl, eps):
    """FastGenModel's x0 student loop ('sde', injected noise) over D.precond_forward in fp64."""
    x = noise.double() * tl[0]
    for i in range(len(tl) - 1):
        x0 = D.precond_forward(sd64, cfg, x, tl[i].expand(noise.shape[0]), lab.double())
        if tl[i + 1] > 0:
            x = x0 + tl[i + 1] * eps[i].double()
    return x0


def test_repack_after_weight_change():
    """After one conv weight and one emb_gain changed in place, the next forward and a graph-replayed few_step_sample captured
    before the change follow the fp64 reference of the NEW weights (and are far from that of the old ones).  Measured on an MI355X:
    forward rel L2 5.2e-6, sampler 9.6e-6; the old weights' outputs lie at 5.5e-2 and 9.8e-2."""
    cfg = D.NARROW
    sd = D.random_state_dict(cfg, seed=1234)
    net = make_net(cfg, sd, compute_dtype="bf16x3")
    B = 2
    x, t, lab = net_inputs(cfg, B, 51)
    noise = torch.randn(B, 3, 64, 64, generator=R.gen(52))
    eps = torch.randn(1, B, 3, 64, 64, generator=R.gen(53))
    tl = torch.tensor([80.0, 1.5, 0.0], dtype=torch.float64)
    sample = lambda: net.few_step_sample(noise.to(dev()), lab.to(dev()), tl, sample_type="sde", eps=eps.to(dev()), use_graph=True).cpu()  # noqa: E731
    with torch.inference_mode():
        old_out = net(x.to(dev()), t.to(dev()), condition=lab.to(dev())).cpu()
        old_s = sample()
        captures, launches = _lib.graph_stats()
        assert torch.equal(sample(), old_s) and _lib.graph_stats() == (captures, launches + 1)
    kw, kg = "unet.enc.32x32_block0.conv_res1.weight", "unet.dec.16x16_block1.emb_gain"
    new = dict(sd)
    new[kw] = sd[kw] + 0.7 * torch.randn(sd[kw].shape, generator=R.gen(54))
    new[kg] = sd[kg] + 0.5
    with torch.no_grad():
        params = dict(net.named_parameters())
        params[kw].copy_(new[kw].to(dev()))
        params[kg].copy_(new[kg].to(dev()))
    sd64 = R.to64(new)
    ref_out = D.precond_forward(sd64, cfg, x.double(), t, lab.double())
    ref_s = sampler_ref(sd64, cfg, noise, lab, tl, eps)
    with torch.inference_mode():
        out = net(x.to(dev()), t.to(dev()), condition=lab.to(dev())).cpu()
        s = sample()
    for what, got, ref, old in (("forward", out, ref_out, old_out), ("sampler", s, ref_s, old_s)):
        moved = ((old.double() - ref).norm() / ref.norm()).item()
        print(f"\nrepack {what}: the old weights' output lies at rel L2 {moved:.2e}")
        assert moved > 100 * TOL["bf16x3"]["rel"], (what, moved)
        check(got, ref, "bf16x3", "repack " + what)


@pytest.mark.parametrize("drop", ["input", "output", "both"])
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_drop_precond(mode, drop):
    """EDM2Precond(drop_precond=...) against the restatement (pinned to the reference by tests/test_edm2_ops_ref.py) under
    tests/test_gpu_edm2.py's TOL.  With 'input' the U-Net's noise label is t itself.  Measured on an MI355X, worst: bf16x3 max_abs
    3.1e-5, rel L2 1.1e-5; bf16 max_abs 1.7e-2, rel L2 5.8e-3."""
    cfg = D.NARROW
    sd = D.random_state_dict(cfg, seed=1234)
    net = make_net(cfg, sd, compute_dtype=mode, drop_precond=drop)
    B = 3
    t = torch.tensor([0.05, 0.7, 2.0], dtype=torch.float64)
    x = torch.randn(B, 3, 64, 64, generator=R.gen(61)) * t.float().reshape(-1, 1, 1, 1)
    lab = labels_for(cfg, B)
    with torch.no_grad():
        want = D.precond_forward(sd, cfg, x, t, lab, drop_precond=drop)
        got = net(x.to(dev()), t.to(dev()), condition=lab.to(dev())).cpu()
    check(got, want, mode, "drop_precond " + drop)
