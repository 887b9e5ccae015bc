"""Per-op and per-block parity of the DhariwalUNet (ADM) kernels (fastgen_amd/csrc/adm.hip) through the fg_op_adm_* entry points and
fg_edm_run_block, each against a plain fp64 torch reference on the CPU, at the shapes and edges where the kernels could go wrong: conv
N / M tails and straddling concats, GroupNorm slots that do not divide hw and groups that straddle the concat, peaked attention whose
maximum sits in the first or the last key tile.  The whole-network tests (test_gpu_dhariwal.py) dilute such errors."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from fastgen_amd import _lib
from fastgen_amd.networks.EDM.network import EDMPrecond

import dhariwal_ref as D

pytestmark = pytest.mark.gpu

MODES = {"bf16": _lib.FG_DTYPE_BF16, "bf16x3": _lib.FG_DTYPE_BF16X3}


def dev():
    return torch.device("cuda:0")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- convolution --------------------------------------------------------------------------------------------------------------

def conv_prologue(x, ab, silu):
    """The conv kernel's operand transform in fp32: fmaf(x, a, b), then SiLU as x / (1 + exp(-x)).  x NCHW fp32, ab [B, C, 2]."""
    if ab is None:
        return x
    a, b = ab[..., 0, None, None].double(), ab[..., 1, None, None].double()
    y = (x.double() * a + b).float()  # one rounding of the exact product-sum: fmaf
    return y / (1.0 + torch.exp(-y)) if silu else y


def mean2x2(x):
    """0.25 (((u00 + u01) + u10) + u11) in fp32, the kernel's order."""
    return 0.25 * (((x[..., 0::2, 0::2] + x[..., 0::2, 1::2]) + x[..., 1::2, 0::2]) + x[..., 1::2, 1::2])


def conv_case_ref(x, ab, silu, res_mode, w, bias, resid, resid_mode, bf16_operands):
    """(fp64 reference, |x'| (*) |w|) of one fg_op_adm_conv call; x NCHW fp32 (the concat), resid NCHW fp32 or None."""
    u = conv_prologue(x, ab, silu)
    if res_mode == 1:
        u = mean2x2(u)
    elif res_mode == 2:
        u = u.repeat_interleave(2, 2).repeat_interleave(2, 3)
    if bf16_operands:  # round to nearest even, as the kernel's bf16 conversions
        u, w = u.bfloat16(), w.bfloat16()
    u, w = u.double(), w.double()
    pad = w.shape[-1] // 2
    ref = F.conv2d(u, w, padding=pad)
    mag = F.conv2d(u.abs(), w.abs(), padding=pad)
    if bias is not None:
        ref = ref + bias.double().reshape(1, -1, 1, 1)
    if resid is not None:
        r = {0: resid, 1: 0.25 * ((resid[..., 0::2, 0::2] + resid[..., 0::2, 1::2]) + (resid[..., 1::2, 0::2] + resid[..., 1::2, 1::2])),
             2: resid.repeat_interleave(2, 2).repeat_interleave(2, 3)}[resid_mode]
        ref = ref + r.double()
    return ref, mag


def run_conv(mode, ks, x1, x2, ab, silu, res_mode, H, w, bias, resid, resid_mode):
    """fg_op_adm_conv on NCHW fp32 CPU tensors; returns NCHW fp32 on the CPU."""
    L = _lib.lib()
    B, C1, Hs = x1.shape[0], x1.shape[1], x1.shape[2]
    C2 = 0 if x2 is None else x2.shape[1]
    cout, cin = w.shape[0], w.shape[1]
    packed = torch.empty(L.fg_op_adm_conv_pack_bytes(mode, cout, cin, ks), dtype=torch.uint8, device=dev())
    wd = w.to(dev()).contiguous()
    _lib.check(L.fg_op_adm_conv_pack(mode, wd.data_ptr(), packed.data_ptr(), cout, cin, ks, None))
    d1 = nhwc(x1).to(dev())
    d2 = None if x2 is None else nhwc(x2).to(dev())
    dab = None if ab is None else ab.to(dev()).contiguous()
    dbias = None if bias is None else bias.to(dev())
    dres = None if resid is None else nhwc(resid).to(dev())
    out = torch.full((B, H, H, cout), float("nan"), device=dev())
    _lib.check(L.fg_op_adm_conv(mode, ks, d1.data_ptr(), C1, ptr(d2), C2, B, Hs, H, res_mode, ptr(dab), silu, packed.data_ptr(),
                                ptr(dbias), ptr(dres), resid_mode, out.data_ptr(), cout, None))
    torch.cuda.synchronize()
    return nchw(out.cpu())


# (res_mode, resid_mode or None, ks, C1, C2, Cout, H (output), B, ab, silu, bias): the 12 res_mode x resid pairs, each run in both
# modes, then single-mode cases for the widest K (9 x 576), H = 64, Cout = 576 with ks = 3 and an affine prologue without SiLU.
PAIRS = [
    (0, None, 3, 96, 32, 64, 16, 3, True, 1, True),
    (0, 0, 1, 64, 0, 200, 8, 1, False, 0, True),
    (0, 1, 3, 64, 0, 96, 8, 3, True, 1, False),
    (0, 2, 3, 32, 0, 3, 32, 1, True, 1, True),
    (1, None, 3, 64, 0, 64, 16, 1, True, 1, True),
    (1, 0, 1, 96, 32, 96, 8, 3, True, 1, False),
    (1, 1, 3, 64, 0, 64, 8, 3, True, 1, True),
    (1, 2, 1, 128, 0, 576, 16, 1, False, 0, True),
    (2, None, 3, 64, 0, 200, 16, 1, True, 1, False),
    (2, 0, 1, 32, 0, 64, 32, 1, False, 0, False),
    (2, 1, 3, 96, 32, 3, 8, 3, True, 1, True),
    (2, 2, 3, 64, 0, 64, 16, 3, True, 1, True),
]
EXTRA = [
    ("bf16", (0, None, 3, 576, 0, 64, 8, 1, False, 0, True)),
    ("bf16x3", (0, None, 3, 576, 0, 64, 8, 1, False, 0, True)),
    ("bf16x3", (0, 0, 3, 64, 0, 64, 64, 1, True, 1, True)),
    ("bf16", (0, 0, 3, 64, 0, 64, 64, 1, False, 0, True)),
    ("bf16x3", (0, None, 3, 64, 0, 576, 8, 3, True, 1, True)),
    ("bf16x3", (0, 0, 1, 128, 0, 192, 16, 1, True, 0, True)),
    ("bf16", (0, 0, 1, 128, 0, 192, 16, 1, True, 0, True)),
]
CONV_CASES = [(m, c) for c in PAIRS for m in ("bf16x3", "bf16")] + EXTRA


def conv_inputs(case, seed):
    res_mode, resid_mode, ks, C1, C2, cout, H, B, with_ab, silu, with_bias = case
    g = gen(seed)
    Hs = {0: H, 1: 2 * H, 2: H // 2}[res_mode]
    x = torch.randn(B, C1 + C2, Hs, Hs, generator=g)
    ab = None
    if with_ab:
        ab = torch.stack([1 + 0.3 * torch.randn(B, C1 + C2, generator=g), 0.3 * torch.randn(B, C1 + C2, generator=g)], dim=-1)
    w = torch.randn(cout, C1 + C2, ks, ks, generator=g) / math.sqrt((C1 + C2) * ks * ks)
    bias = 0.1 * torch.randn(cout, generator=g) if with_bias else None
    resid = None
    if resid_mode is not None:
        R = {0: H, 1: 2 * H, 2: H // 2}[resid_mode]
        resid = torch.randn(B, cout, R, R, generator=g)
    return x, ab, w, bias, resid


def conv_errors(mode, case, seed):
    """(|got - ref|, bf16x3 bound, bound of the mode, |got - exact|) for one case; ref rounds the operands to bf16 in the bf16 mode,
    exact never does."""
    res_mode, resid_mode, ks, C1, C2, cout, H, B, with_ab, silu, with_bias = case
    x, ab, w, bias, resid = conv_inputs(case, seed)
    got = run_conv(MODES[mode], ks, x[:, :C1], x[:, C1:] if C2 else None, ab, silu, res_mode, H, w, bias, resid, resid_mode or 0)
    assert torch.isfinite(got).all()
    bf16 = mode == "bf16"
    ref, mag = conv_case_ref(x, ab, silu, res_mode, w, bias, resid, resid_mode, bf16)
    err = (got.double() - ref).abs()
    exact, exact_mag = conv_case_ref(x, ab, silu, res_mode, w, bias, resid, resid_mode, False)
    x3_bound = 2.0 ** -15 * exact_mag + 1e-6
    if not bf16:
        bound = x3_bound
    elif ab is None:
        bound = 2.0 ** -17 * mag  # operands rounded identically: only the fp32 accumulation differs
    else:
        bound = 2.0 ** -7 * mag  # the fp32 prologue can land on the other side of a bf16 rounding tie
    return err, x3_bound, bound, (got.double() - exact).abs()


@pytest.mark.parametrize("mode,case", CONV_CASES, ids=[f"{m}-{'-'.join(map(str, c))}" for m, c in CONV_CASES])
def test_conv(mode, case):
    """Measured on an MI355X, worst max err / bound over the cases: bf16x3 0.21, bf16 without prologue 0.017, bf16 with prologue 0.007."""
    err, _, bound, _ = conv_errors(mode, case, seed=sum(int(v or 0) for v in case))
    ratio = (err / bound).max().item()
    print(f"\nconv {mode} {case}: max err {err.max().item():.3e}, max err/bound {ratio:.3f}")
    assert ratio <= 1.0, (mode, case, ratio)


@pytest.mark.parametrize("ks", [1, 3])
def test_conv_bound_tells_bf16_from_bf16x3(ks):
    """The bf16x3 tolerance is tight enough to see a lost lo product: the bf16 mode's output breaks it (measured: 79x the bound at
    ks = 1, 33x at ks = 3)."""
    case = (0, None, ks, 64, 0, 64, 16, 1, True, 1, True)
    _, x3_bound, _, err = conv_errors("bf16", case, seed=7)
    ratio = (err / x3_bound).max().item()
    print(f"\nconv bf16 against the bf16x3 bound, ks {ks}: max err/bound {ratio:.1f}")
    assert ratio > 2.0, ratio


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------

# (C1, C2, hw, temb, offset, B): C = 64 .. 1536 (group sizes 4, 6, 12, 24, 42, 48), concats whose boundary falls inside a group
# (160 + 32 in groups of 6, 768 + 576 in groups of 42), hw of one slot (64, 127) and slots that do not divide hw (200)
GN_CASES = [
    (64, 0, 4096, True, 0, 2),
    (64, 0, 64, False, 16, 3),
    (192, 0, 127, True, 4, 2),
    (160, 32, 200, True, 16, 2),
    (160, 32, 128, False, 0, 1),
    (384, 0, 1024, False, 4, 1),
    (384, 0, 128, True, 0, 3),
    (768, 0, 64, True, 16, 2),
    (768, 576, 127, False, 4, 1),
    (1344, 0, 128, True, 16, 1),
    (1536, 0, 64, False, 0, 2),
    (1536, 0, 200, True, 4, 1),
    (192, 0, 4096, False, 16, 1),
    (96, 32, 1024, True, 0, 2),
]


@pytest.mark.parametrize("c1,c2,hw,with_temb,offset,B", GN_CASES)
def test_gn_coeffs(c1, c2, hw, with_temb, offset, B):
    """y = a x + b from the kernel's coefficients against fp64 group_norm + the adaptive fold.  Measured worst |dy| / (1 + |y|):
    offset <= 4: 3.5e-6, offset 16: 5.0e-5 (fp32 sums of squares over 64-pixel slots)."""
    L = _lib.lib()
    C = c1 + c2
    g = gen(c1 * 7 + c2 + hw)
    x = offset + torch.randn(B, hw, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    stride = 2 * C + 40
    temb = 0.1 * torch.randn(B, stride, generator=g) if with_temb else None
    d1, d2 = x[..., :c1].contiguous().to(dev()), x[..., c1:].contiguous().to(dev()) if c2 else None
    ws = torch.empty(L.fg_op_adm_gn_workspace_bytes(B, hw, C), dtype=torch.uint8, device=dev())
    ab = torch.full((B, C, 2), float("nan"), device=dev())
    dg, db = gamma.to(dev()), beta.to(dev())
    dt = None if temb is None else temb.to(dev())
    _lib.check(L.fg_op_adm_gn_coeffs(d1.data_ptr(), c1, ptr(d2), c2, dg.data_ptr(), db.data_ptr(), 1e-5, ptr(dt), stride, ab.data_ptr(),
                                     B, hw, ws.data_ptr(), ws.numel(), None))
    ab = ab.cpu().double()
    xd = x.double()
    y = ab[:, None, :, 0] * xd + ab[:, None, :, 1]
    ref = F.group_norm(xd.transpose(1, 2), min(32, C // 4), gamma.double(), beta.double(), 1e-5).transpose(1, 2)
    if temb is not None:
        scale, shift = temb[:, :C].double(), temb[:, C:2 * C].double()
        ref = shift[:, None] + ref * (scale[:, None] + 1)
    rel = ((y - ref).abs() / (1 + ref.abs())).max().item()
    print(f"\ngn C1={c1} C2={c2} hw={hw} temb={with_temb} offset={offset}: max |dy|/(1+|y|) {rel:.2e}")
    assert rel <= (5e-6 if offset <= 4 else 1e-4), rel


# ---- attention ----------------------------------------------------------------------------------------------------------------

def attention_inputs(B, T, heads, scale, kind, seed):
    """q, k, v [B, heads, T, 64].  random: logits q.k/8 of standard deviation ~scale; last / first: every query's largest logit sits in
    the last / first 32-key tile (a boost along channel 0, which the noise leaves out); uniform: all keys equal (equal logits)."""
    g = gen(seed)
    s = math.sqrt(scale)
    q = s * torch.randn(B, heads, T, 64, generator=g)
    k = s * torch.randn(B, heads, T, 64, generator=g)
    v = torch.randn(B, heads, T, 64, generator=g)
    if kind in ("last", "first"):
        k[..., 0] = 0
        a = math.sqrt(8 * (8 + 6 * scale))  # a^2 / 8: the tile's logit lead, 6 noise deviations and more
        q[..., 0] = a
        tile = slice(T - 32, T) if kind == "last" else slice(0, 32)
        k[:, :, tile, 0] = a * (0.75 + 0.25 * torch.rand(B, heads, 32, generator=g))
    elif kind == "uniform":
        k[:] = k[:, :, :1]
    return q, k, v


ATTN_CASES = [  # (B, T, heads, logit scale, kind)
    (1, 64, 1, 1, "random"),
    (2, 256, 3, 8, "random"),
    (1, 1024, 12, 30, "random"),
    (2, 1024, 3, 1, "last"),
    (1, 1024, 1, 8, "last"),
    (1, 256, 3, 30, "last"),
    (1, 256, 12, 8, "first"),
    (2, 256, 1, 30, "first"),
    (2, 64, 3, 1, "uniform"),
    (1, 1024, 1, 8, "uniform"),
]


@pytest.mark.parametrize("B,T,heads,scale,kind", ATTN_CASES)
def test_attention(B, T, heads, scale, kind):
    """Against fp64 softmax attention: |d| <= max|v| (4e-6 + 1e-6 max_k(|q|.|k|) / 8) per query.  Measured worst ratio: 0.11."""
    L = _lib.lib()
    q, k, v = attention_inputs(B, T, heads, scale, kind, seed=T + heads + int(scale))
    logits = torch.einsum("bhqc,bhkc->bhqk", q.double(), k.double()) / 8
    if kind in ("last", "first"):
        want = T // 32 - 1 if kind == "last" else 0
        assert (logits.argmax(-1) // 32 == want).all()
    ref = torch.einsum("bhqk,bhkc->bhqc", logits.softmax(-1), v.double())
    # qkv [B, T, heads * 192]: channel h * 192 + 3 c + j, j = q, k, v
    qkv = torch.stack([q, k, v], dim=-1).permute(0, 2, 1, 3, 4).reshape(B, T, heads * 192).contiguous().to(dev())
    out = torch.full((B, T, heads * 64), float("nan"), device=dev())
    _lib.check(L.fg_op_adm_attention(qkv.data_ptr(), out.data_ptr(), B, T, heads, None))
    got = out.cpu().double().reshape(B, T, heads, 64).transpose(1, 2)
    mag = torch.einsum("bhqc,bhkc->bhqk", q.double().abs(), k.double().abs()).amax(-1, keepdim=True) / 8
    vmax = v.abs().amax(dim=(2, 3), keepdim=True).double()
    bound = vmax * (4e-6 + 1e-6 * mag)
    ratio = ((got - ref).abs() / bound).max().item()
    print(f"\nattention B={B} T={T} heads={heads} scale={scale} {kind}: max err/bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


def test_attention_refuses_partial_tiles():
    L = _lib.lib()
    buf = torch.zeros(2 * 96 * 192, device=dev())
    assert L.fg_op_adm_attention(buf.data_ptr(), buf.data_ptr(), 1, 96, 1, None) == 1


# ---- mapping-network input ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,with_aug", [(64, True), (64, False), (192, True)])
def test_map_in(n, with_aug):
    """c_noise = log(sigma) / 4 over sigma in [0.002, 80], against D.positional_embedding + map_augment in fp64.  Measured worst: 7.9e-7."""
    L = _lib.lib()
    B = 64
    g = gen(n)
    c_noise = (torch.exp(torch.linspace(math.log(0.002), math.log(80.0), B, dtype=torch.float64)).log() / 4).float()
    half = n // 2
    freqs = (1 / 10000) ** (torch.arange(0, half, dtype=torch.float32) / half)
    aug = torch.randn(B, 9, generator=g) if with_aug else None
    wa = torch.randn(n, 9, generator=g) / 3 if with_aug else None
    dc, df = c_noise.to(dev()), freqs.to(dev())
    daug, dwa = (aug.to(dev()), wa.to(dev())) if with_aug else (None, None)
    out = torch.full((B, n), float("nan"), device=dev())
    _lib.check(L.fg_op_adm_map_in(dc.data_ptr(), df.data_ptr(), ptr(daug), ptr(dwa), 9, out.data_ptr(), B, n, None))
    ref = D.positional_embedding(c_noise.double(), n)
    if with_aug:
        ref = ref + aug.double() @ wa.double().t()
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"\nmap_in n={n} aug={with_aug}: max err {err:.2e}")
    assert err <= 2e-6, err


# ---- whole UNetBlocks through fg_edm_run_block --------------------------------------------------------------------------------

def run_blocks(cfg, B, mode, seed):
    """Every block of cfg through fg_edm_run_block, against D.unet_block in fp64; returns [(key, max|d| / max|ref|, rel L2)]."""
    sd = D.random_state_dict(cfg, seed=seed)
    net = EDMPrecond(**cfg.kwargs(), compute_dtype=mode)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev()).eval().requires_grad_(False)
    L = _lib.lib()
    _, enc, dec = D.layout(cfg)
    blocks = [("enc", b) for b in enc] + [("dec", b) for b in dec]
    E = cfg.model_channels * cfg.channel_mult_emb
    g = gen(seed + 1)
    emb = torch.randn(B, E, generator=g)
    demb = emb.to(dev())
    res = []
    with torch.inference_mode():
        dt, h = net._engine(dev())
        ws = net._workspace(dt, h, B, dev())
        assert L.fg_edm_num_blocks(h) == len(blocks)
        prev = None
        for i, (side, b) in enumerate(blocks):
            ri = ctypes.c_int()
            _lib.check(L.fg_edm_block_info(h, i, None, None, None, ctypes.byref(ri), None, None))
            c2 = b.cin - prev if side == "dec" and b.cin != prev else 0
            prev = b.cout
            x = torch.randn(B, b.cin, ri.value, ri.value, generator=g)
            c1 = b.cin - c2
            x1, x2 = nhwc(x[:, :c1]).to(dev()), nhwc(x[:, c1:]).to(dev()) if c2 else None
            out = torch.full((B, b.res, b.res, b.cout), float("nan"), device=dev())
            _lib.check(L.fg_edm_run_block(h, i, x1.data_ptr(), c1, ptr(x2), c2, demb.data_ptr(), out.data_ptr(), B, ws.data_ptr(),
                                          ws.numel(), None))
            prefix = f"model.{side}.{b.key}."
            bsd = {k: v.double() for k, v in sd.items() if k.startswith(prefix)}
            ref = D.unet_block(bsd, f"model.{side}", b, x.double(), emb.double())
            got = nchw(out.cpu()).double()
            assert torch.isfinite(got).all(), b.key
            d = got - ref
            res.append((f"{side}.{b.key}", (d.abs().max() / ref.abs().max()).item(), (d.norm() / ref.norm()).item()))
    del net
    torch.cuda.empty_cache()
    return res


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_blocks_narrow(mode):
    """Every NARROW block at B = 3.  Measured worst: bf16x3 max|d| / max|ref| 6.2e-6, bf16 rel L2 2.8e-3."""
    res = run_blocks(D.NARROW, 3, mode, seed=99)
    for key, mx, rel in res:
        print(f"\nblock narrow {mode} {key}: max|d|/max|ref| {mx:.2e} rel L2 {rel:.2e}")
    for key, mx, rel in res:
        if mode == "bf16x3":
            assert mx <= 2e-5, (key, mx)
        else:
            assert rel <= 5e-3, (key, rel)


def test_blocks_in64():
    """Every IN64 block at B = 1 in bf16x3.  Measured worst max|d| / max|ref|: 6.7e-6."""
    res = run_blocks(D.IN64, 1, "bf16x3", seed=98)
    assert len(res) == 36
    for key, mx, rel in res:
        print(f"\nblock in64 bf16x3 {key}: max|d|/max|ref| {mx:.2e} rel L2 {rel:.2e}")
    for key, mx, rel in res:
        assert mx <= 2e-5, (key, mx)
