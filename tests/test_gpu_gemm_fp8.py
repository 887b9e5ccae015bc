"""The fp8 (e4m3fn) token GEMM and its quantisers (fastgen_amd/csrc/gemm.hip `fg_op_gemm_fp8`, `fg_op_quant_rows_fp8`; dit.hip
`fg_op_dit_ln_modulate_fp8`) on the GPU.

Exact: integer operands in [-8, 8] (exact in e4m3), power-of-two row / channel scales in {1/2, 1, 2} and integer biases make every
partial sum an integer multiple of 1/4 below 2^22 - exact in fp32 in any order - so the result must EQUAL the fp64 result rounded to
bf16.  The operand patterns are asymmetric in (row, k) and differ between A and W: a lane map of v_mfma_scale_f32_16x16x128_f8f6f4 that
pairs the wrong k bytes, a swapped octet plane or a transposed tile changes integers, not roundings.
General: Gaussian operands quantised by the mirror (tests/dit_fp8_ref.py); `want` is the fp64 product of the same dequantised operands,
so - as in tests/test_gemm.py - only the accumulation order and the bf16 rounding of the output differ: |got - want| <= 2^-8 max |want|
+ 1e-6 (+ 1e-3 where GELU, gate or residual arithmetic runs in fp32 on the way)."""
import ctypes

import pytest
import torch

import dit_fp8_ref as Q

gpu = pytest.mark.gpu

_SHAPES = [(256, 256, 128), (512, 192, 256), (77, 3456, 1152), (513, 384, 384), (300, 64, 256), (1000, 1152, 1152), (2048, 1152, 4608)]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _gemm(qa, sa, qw, sw, bias=None, act=0, gate=None, gate_stride=0, gate_rows=1, resid=None, order=1, out=None):
    from fastgen_amd import _lib

    m, k = qa.shape
    n = qw.shape[0]
    if out is None:
        out = torch.empty(m, n, dtype=torch.bfloat16, device=qa.device)
    _lib.check(_lib.lib().fg_op_gemm_fp8(_p(qa), _p(qw), _p(bias), _p(out), m, n, k, act, _p(gate), gate_stride, gate_rows, _p(resid), order,
                                         _p(sa), _p(sw), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out


def _want(qa, sa, qw, sw, bias=None, act=0, gate=None, gate_rows=1, resid=None):
    """fp64 on the dequantised operands (on the device: a 2048 x 1152 x 4608 fp64 product is seconds on the host)."""
    wide = lambda q: q.cpu().float().double().cuda()  # noqa: E731  (e4m3 -> fp64 is exact; widened on the host)
    v = (wide(qa) * sa.double().unsqueeze(1)) @ (wide(qw) * sw.double().unsqueeze(1)).t()
    if bias is not None:
        v = v + bias.double()
    if act == 1:
        v = torch.nn.functional.gelu(v, approximate="tanh")
    if gate is not None:
        v = v * gate.double().repeat_interleave(gate_rows, dim=0)[: v.shape[0]]
    if resid is not None:
        v = v + resid.double()
    return v


def _int_pattern(rows, k, a, b, c, mod):
    """integers in [-8, 8], asymmetric in (row, k): ((a r + b k + (r k) % mod) % 17) - 8"""
    r = torch.arange(rows, dtype=torch.int64).unsqueeze(1)
    kk = torch.arange(k, dtype=torch.int64).unsqueeze(0)
    return (((a * r + b * kk + (r * kk) % mod) % 17) - 8).float()


@gpu
@pytest.mark.parametrize("order", [1, 16 + 1], ids=["auto", "register-staged"])
@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_integer_products(shape, order):
    m, n, k = shape
    a = _int_pattern(m, k, 3, 5, 7, 7)
    w = _int_pattern(n, k, 7, 11, 1, 5)
    sa = 2.0 ** ((torch.arange(m) % 3) - 1).float()
    sw = 2.0 ** (((torch.arange(n) * 5) % 3) - 1).float()
    bias = ((torch.arange(n) * 7) % 9 - 4).float()
    qa, qw = a.to(torch.float8_e4m3fn).cuda(), w.to(torch.float8_e4m3fn).cuda()
    assert torch.equal(qa.cpu().float(), a) and torch.equal(qw.cpu().float(), w)
    sa, sw, bias = sa.cuda(), sw.cuda(), bias.cuda()
    got = _gemm(qa, sa, qw, sw, bias, order=order)
    want = _want(qa, sa, qw, sw, bias)
    assert float(want.abs().max()) < 2 ** 22
    assert torch.equal(got, want.to(torch.bfloat16)), (shape, order, float((got.double() - want).abs().max()))


@gpu
@pytest.mark.parametrize("order", [1, 16 + 1], ids=["auto", "register-staged"])
def test_exact_selection_matrix(order):
    """A selects one k per row: out[m][n] = a_scale[m] w_scale[n] W[n][k(m)] - the k byte of A that a lane holds must meet the SAME k byte of W."""
    m, n, k = 513, 384, 384
    sel = (torch.arange(m) * 37 + 5) % k
    a = torch.zeros(m, k)
    a[torch.arange(m), sel] = 1.0
    w = _int_pattern(n, k, 7, 11, 1, 5)
    sa = (2.0 ** ((torch.arange(m) % 3) - 1).float()).cuda()
    sw = (2.0 ** (((torch.arange(n) * 5) % 3) - 1).float()).cuda()
    got = _gemm(a.to(torch.float8_e4m3fn).cuda(), sa, w.to(torch.float8_e4m3fn).cuda(), sw, order=order)
    want = (w[:, sel].t().cuda() * sa.unsqueeze(1) * sw.unsqueeze(0)).to(torch.bfloat16)
    assert torch.equal(got, want)


def _gauss(m, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, k, generator=g) * (0.5 + 4.0 * torch.rand(m, 1, generator=g))      # rows (and channels) of different scale
    w = torch.randn(n, k, generator=g) * k ** -0.5 * (0.5 + 4.0 * torch.rand(n, 1, generator=g))
    qa, sa = Q.quant_rows(a)
    qw, sw = Q.quant_rows(w)
    return qa.cuda(), sa.cuda(), qw.cuda(), sw.cuda(), g


@gpu
@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_general_against_fp64_on_the_same_operands(shape):
    m, n, k = shape
    qa, sa, qw, sw, g = _gauss(m, n, k, m * 7 + n * 3 + k)
    bias = torch.randn(n, generator=g).cuda()
    got = _gemm(qa, sa, qw, sw, bias)
    want = _want(qa, sa, qw, sw, bias)
    err, top = float((got.double() - want).abs().max()), float(want.abs().max())
    print(f"\n[gemm-fp8] {shape}: max err {err:.3e} = {err / top:.2e} of max |want| {top:.2f}")
    assert err <= 2 ** -8 * top + 1e-6, (shape, err, top)
    assert torch.equal(_gemm(qa, sa, qw, sw, bias), got)  # the same bits on a second run


@gpu
@pytest.mark.parametrize("shape,order", [((1000, 1152, 1152), 1), ((1000, 1152, 1152), 16 + 1), ((513, 384, 384), 1), ((300, 64, 256), 1)],
                         ids=["pp", "register-staged", "pp-ragged", "narrow"])
def test_epilogues(shape, order):
    m, n, k = shape
    rows = 256
    qa, sa, qw, sw, g = _gauss(m, n, k, 5 + m)
    bias = torch.randn(n, generator=g).cuda()
    gate = torch.randn((m + rows - 1) // rows, 6 * n, generator=g).cuda()[:, 2 * n: 3 * n]  # a chunk of the adaLN vector: strided rows
    resid = torch.randn(m, n, generator=g).bfloat16().cuda()
    got = _gemm(qa, sa, qw, sw, bias, act=1, order=order)
    want = _want(qa, sa, qw, sw, bias, act=1)
    assert float((got.double() - want).abs().max()) <= 2 ** -8 * float(want.abs().max()) + 1e-3
    got = _gemm(qa, sa, qw, sw, bias, gate=gate, gate_stride=6 * n, gate_rows=rows, resid=resid, order=order)
    want = _want(qa, sa, qw, sw, bias, gate=gate, gate_rows=rows, resid=resid)
    assert float((got.double() - want).abs().max()) <= 2 ** -8 * float(want.abs().max()) + 1e-3
    # in place on the residual stream, as the engine runs proj and fc2
    x = resid.clone()
    _gemm(qa, sa, qw, sw, bias, gate=gate, gate_stride=6 * n, gate_rows=rows, resid=x, order=order, out=x)
    assert torch.equal(x, got)


@gpu
@pytest.mark.parametrize("k", [128, 384, 1152, 4608])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_quant_rows_is_the_mirror_bit_for_bit(dtype, k):
    from fastgen_amd import _lib

    m = 261  # not a multiple of the 4 rows per workgroup
    g = torch.Generator().manual_seed(k + (1 if dtype == torch.bfloat16 else 0))
    x = torch.randn(m, k, generator=g) * torch.exp(3.0 * torch.randn(m, 1, generator=g))
    x[3] = 0.0                       # a zero row
    x[5, 7:] *= 1e-4                 # values deep in the subnormals of the row's scale
    x[9, 0] = 448.0                  # amax exactly 448
    x[9, 1:] = x[9, 1:].clamp(-400, 400)
    x = x.to(dtype)
    xd = x.cuda()
    q = torch.empty(m, k, dtype=torch.uint8, device="cuda")
    s = torch.empty(m, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().fg_op_quant_rows_fp8(1 if dtype == torch.bfloat16 else 0, _p(xd), _p(q), _p(s), m, k,
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    qm, sm = Q.quant_rows(x)
    assert torch.equal(s.cpu(), sm)
    diff = (q.cpu() != qm.view(torch.uint8))
    assert not diff.any(), (int(diff.sum()), diff.nonzero()[:4].tolist())


@gpu
@pytest.mark.parametrize("d", [384, 768, 1024, 1152])
def test_ln_modulate_fp8(d):
    from fastgen_amd import _lib

    ntok, tpi = 300, 256  # two images; a ragged last workgroup (16 tokens each)
    g = torch.Generator().manual_seed(d)
    x = (torch.randn(ntok, d, generator=g) * 2 + 0.3 * torch.randn(ntok, 1, generator=g)).bfloat16()
    mod = 0.5 * torch.randn(2, 6 * d, generator=g)
    shift_off, scale_off = 3 * d, 4 * d
    xd, md = x.cuda(), mod.cuda()
    y8 = torch.empty(ntok, d, dtype=torch.uint8, device="cuda")
    ys = torch.empty(ntok, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().fg_op_dit_ln_modulate_fp8(_p(xd), _p(md), 6 * d, shift_off, scale_off, _p(y8), _p(ys), ntok, d, tpi,
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    x64, m64 = x.double(), mod.double().repeat_interleave(tpi, dim=0)[:ntok]
    y = torch.nn.functional.layer_norm(x64, (d,), eps=1e-6) * (1 + m64[:, scale_off: scale_off + d]) + m64[:, shift_off: shift_off + d]
    amax = y.abs().amax(dim=1)
    scale = ys.cpu().double()
    ulp = (scale.float().abs().frexp().exponent.double() - 24).exp2()  # fp32 ulp at the scale's binade
    worst = float(((scale - amax / 448.0).abs() / ulp).max())
    deq = y8.cpu().view(torch.float8_e4m3fn).double() * scale.unsqueeze(1)
    bound = 2.0 ** -4 * y.abs() + scale.unsqueeze(1) * 2.0 ** -10 + 1e-5 * amax.unsqueeze(1)
    print(f"\n[ln-fp8] d {d}: scale off by {worst:.2f} ulp at most; max (|deq - y| / bound) {float(((deq - y).abs() / bound).max()):.3f}")
    assert worst <= 4.0, worst
    assert ((deq - y).abs() <= bound).all()


def test_refusals():
    """K % 128 != 0, N % 16 != 0 and act = 2 are FG_EINVAL before any launch (no GPU needed: nothing is dereferenced)."""
    from fastgen_amd import _lib

    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64)
    for m, n, k, act in ((512, 1152, 1088, 0), (512, 1152, 64, 0), (512, 1160, 1152, 0), (512, 1152, 1152, 2)):
        assert L.fg_op_gemm_fp8(p, p, None, p, m, n, k, act, None, 0, 1, None, 1, p, p, None) == 1, (m, n, k, act)
        assert b"fg_op_gemm_fp8" in L.fg_last_error()
