"""Token GEMM of the transformer blocks in the split-bf16 mode (fastgen_amd/csrc/gemm.hip `launch_gemm_x3`, through `fg_op_gemm_x3`):
the four linears of every DiT block in the bf16x3 compute mode, the DiT's default.  fp32 operands are split into bf16 hi / lo planes
and contracted as a_hi w_hi + a_hi w_lo + a_lo w_hi with fp32 accumulation, with the fused epilogues the engine uses: fp32 out with
adaLN gate x value + residual (GM_EPI_TOK32), GELU(tanh) written as [hi | lo] bf16 planes (GM_EPI_SPLIT; the head-split epilogue is
pinned through tests/test_gpu_dit_blocks.py).  Checked elementwise against fp64 on the same fp32 operands with the bound of the
split-bf16 arithmetic, |got - ref| <= 2^-15 (|a| @ |w|^T + |bias|), carried through GELU, gate and residual (the style of the ADM
conv test, test_gpu_adm_ops.py), at the DiT-S / DiT-XL shapes, ragged token counts, in place, and across the launcher's row cutting
(rows_max = 2^31 / (4 K): at K = 4 608 a second launch starts at row 116 480 = image 455)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _x3(a, w, bias=None, act=0, gate=None, gate_stride=0, gate_rows=256, resid=None, out_mode=0, out=None):
    from fastgen_amd import _lib

    m, k = a.shape
    n = w.shape[0]
    if out is None:
        out = torch.empty(m, n, device=a.device) if out_mode == 0 else torch.empty(m, 2 * n, dtype=torch.bfloat16, device=a.device)
    _lib.check(_lib.lib().fg_op_gemm_x3(_p(a), _p(w), _p(bias), _p(out), m, n, k, act, _p(gate), gate_stride, gate_rows, _p(resid),
                                        out_mode, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    if out_mode == 1:  # [hi | lo] planes -> the fp32 value they carry (exact in fp64)
        return out[:, :n].double() + out[:, n:].double(), out
    return out.double(), out


def _ref(a, w, bias=None, act=0, gate=None, gate_rows=256, resid=None, out_mode=0):
    """(fp64 value, elementwise bound) of one call; a, w ... on the CPU; gate [rows][n] as the kernel indexes it."""
    a, w = a.double(), w.double()
    v = a @ w.t()
    mag = a.abs() @ w.abs().t()
    if bias is not None:
        v, mag = v + bias.double(), mag + bias.double().abs()
    bound = 2.0 ** -15 * mag
    if act == 1:
        v = torch.nn.functional.gelu(v, approximate="tanh")
        bound = 1.2 * bound  # |d/dx GELU_tanh| <= 1.13
    if gate is not None:
        gr = gate.double().repeat_interleave(gate_rows, dim=0)[: v.shape[0]]
        v, bound = v * gr, bound * gr.abs()
    if resid is not None:
        v = v + resid.double()
    # fp32 roundings of the epilogue; [hi | lo] planes hold the fp32 value to 2^-17 of itself
    bound = bound + (2.0 ** -22 + (2.0 ** -17 if out_mode == 1 else 0.0)) * v.abs() + 1e-30
    return v, bound


def _operands(m, n, k, seed, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) * k ** -0.5
    bias = 0.1 * torch.randn(n, generator=g)
    mod = torch.randn((m + 255) // 256, 6 * n, generator=g)  # the adaLN vectors [images][6 n]: shift, scale, gate x 2
    resid = torch.randn(m, n, generator=g)
    return a, w, bias, mod, resid


def _ratio(got, ref, bound):
    return ((got.cpu() - ref).abs() / bound).max().item()


_DIT = {"S": (384, 1536), "XL": (1152, 4608)}


@pytest.mark.parametrize("arch", ["S", "XL"])
@pytest.mark.parametrize("m", [512, 257, 300, 513])
def test_block_linears(arch, m):
    """qkv (plain fp32 out), proj (gate of period 256 tokens at the engine's offset 2 D in rows of 6 D, + residual), fc1 (GELU, [hi | lo]
    planes) and fc2 (gate at 5 D + residual) of one DiT block."""
    D, Hd = _DIT[arch]
    worst = {}
    for name, n, k, act, goff, out_mode in (("qkv", 3 * D, D, 0, None, 0), ("proj", D, D, 0, 2, 0), ("fc1", Hd, D, 1, None, 1),
                                              ("fc2", D, Hd, 0, 5, 0)):
        a, w, bias, mod, resid = _operands(m, n, k, seed=m + n + k)
        gate = mod[:, goff * n: (goff + 1) * n] if goff is not None else None
        resid = resid if goff is not None else None
        modd = mod.cuda()
        got, raw = _x3(a.cuda(), w.cuda(), bias.cuda(), act, modd[:, goff * n:] if goff is not None else None, 6 * n, 256,
                       resid.cuda() if resid is not None else None, out_mode)
        ref, bound = _ref(a, w, bias, act, gate, 256, resid, out_mode)
        worst[name] = _ratio(got, ref, bound)
        if out_mode == 1:  # lo is the rounding remainder of hi: |lo| <= ulp(hi) / 2
            hi, lo = raw[:, :n].double().cpu(), raw[:, n:].double().cpu()
            half_ulp = torch.where(hi == 0, torch.zeros_like(hi), torch.exp2(torch.floor(torch.log2(hi.abs())) - 8))
            assert (lo.abs() <= half_ulp).all(), name
    print(f"\ngemm x3 {arch} m={m}: max err/bound " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_in_place_residual():
    """out == resid (the engine's x + gate * branch is written over a buffer it reads; shifted ragged tiles store their overlap once)."""
    m, n, k = 513, 1152, 1152
    a, w, bias, mod, resid = _operands(m, n, k, seed=3)
    x = resid.cuda()
    got, _ = _x3(a.cuda(), w.cuda(), bias.cuda(), 0, mod.cuda()[:, 2 * n:], 6 * n, 256, x, 0, out=x)
    ref, bound = _ref(a, w, bias, 0, mod[:, 2 * n: 3 * n], 256, resid)
    assert _ratio(got, ref, bound) <= 1.0


def test_row_cutting_across_launches():
    """k = 4 608 (DiT-XL fc2): rows_max = 2^31 / (4 k) rounded to whole tiles = 116 480, so m = 116 736 runs as two launches, the
    second with row0 = 116 480 (its gate rows and residual offsets).  Operands generated on the device; the 512 rows around the cut
    checked against fp64."""
    m, n, k, cut = 116736, 1152, 4608, 116480
    g = torch.Generator(device="cuda").manual_seed(11)
    a = torch.randn(m, k, device="cuda", generator=g)
    w = torch.randn(n, k, device="cuda", generator=g) * k ** -0.5
    bias = 0.1 * torch.randn(n, device="cuda", generator=g)
    mod = torch.randn(m // 256, 6 * n, device="cuda", generator=g)
    resid = torch.randn(m, n, device="cuda", generator=g)
    got, _ = _x3(a, w, bias, 0, mod[:, 5 * n:], 6 * n, 256, resid, 0)
    rows = slice(cut - 256, cut + 256)
    ref, bound = _ref(a[rows].cpu(), w.cpu(), bias.cpu(), 0, mod[(cut - 256) // 256: (cut + 256) // 256, 5 * n:].cpu(), 256,
                      resid[rows].cpu())
    ratio = _ratio(got[rows], ref, bound)
    print(f"\ngemm x3 row cut at {cut}: max err/bound {ratio:.3f}")
    assert ratio <= 1.0


def test_bound_tells_bf16_from_bf16x3():
    """The bound is tight enough to see a lost lo product: the bf16 GEMM (fg_op_gemm_bf16) on the same operands breaks it (measured:
    29x the bound; the split-bf16 GEMM's worst over this file is 0.23 of it)."""
    from fastgen_amd import _lib

    m, n, k = 512, 1152, 1152
    a, w, bias, _, _ = _operands(m, n, k, seed=5)
    ref, bound = _ref(a, w, bias)
    got, _ = _x3(a.cuda(), w.cuda(), bias.cuda())
    assert _ratio(got, ref, bound) <= 1.0
    out = torch.empty(m, n, dtype=torch.bfloat16, device="cuda")
    ab, wb, bd = a.bfloat16().cuda(), w.bfloat16().cuda(), bias.cuda()
    _lib.check(_lib.lib().fg_op_gemm_bf16(_p(ab), _p(wb), _p(bd), _p(out), m, n, k, 0, None, 0, 1, None, 1,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    ratio = _ratio(out.double(), ref, bound)
    print(f"\ngemm bf16 against the bf16x3 bound: max err/bound {ratio:.1f}")
    assert ratio > 10.0
