"""The fp8 (e4m3fn, W8A8) compute mode of the DiT without a GPU: the torch mirror of the row quantiser at its edges, how far the
quantisation itself moves the network (the fake-quant oracle of tests/dit_fp8_ref.py against the reference-recorded golden output: the
yardstick of tests/test_gpu_dit_fp8.py), and which modules accept the mode."""
import ctypes
import os

import pytest
import torch

import dit_fp8_ref as Q
from oracle import dit_ref as R

CFGS = {"xl": R.XL_2, "s": R.S_2}


def test_mirror_zero_row_and_full_scale():
    x = torch.zeros(3, 128)
    x[1, 5], x[1, 77] = 3.0, -1.5
    x[2, :] = torch.linspace(-1, 1, 128)
    q, s = Q.quant_rows(x)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32
    assert s[0].item() == 1.0 and torch.equal(q[0].float(), torch.zeros(128))           # a zero row: scale 1, q 0
    assert s[1].item() == torch.tensor(3.0).div(torch.tensor(448.0)).item()              # amax / 448 as an fp32 division
    assert q[1, 5].float().item() == 448.0 and q[1, 77].float().item() == -224.0         # amax lands on +-448 exactly
    assert q[2, 0].float().item() == -448.0 and q[2, 127].float().item() == 448.0
    assert torch.isfinite(q.float()).all()
    # amax * (448 / amax) can round to just above 448: the clamp keeps it finite (e4m3fn has no inf; 464 and up would be NaN)
    for v in (0.3, 1e-3, 7.77, 123.456, 3e4, 1.0000001):
        q1, _ = Q.quant_rows(torch.tensor([[v] + [0.0] * 127]))
        assert q1[0, 0].float().item() == 448.0, v


def test_mirror_rounding_and_subnormals():
    # amax = 448: scale 1, inv 1 - the row is converted as it stands
    x = torch.zeros(1, 128)
    x[0, 0] = 448.0
    x[0, 1:9] = torch.tensor([2.0 ** -10, 3 * 2.0 ** -11, 2.0 ** -9, 2.0 ** -6, 17.0, 19.0, 1.0625, 1.1875])
    q, s = Q.quant_rows(x)
    assert s.item() == 1.0
    got = q[0, 1:9].float().tolist()
    # 2^-10 is half the smallest subnormal (2^-9) and ties to even: 0; 3 * 2^-11 = 0.75 of it rounds up to 2^-9; 2^-6 is the smallest
    # normal; 17 and 19 tie between 16, 18, 20 -> the even mantissas 16 and 20; 1.0625 -> 1.0 and 1.1875 -> 1.25 (ties to even)
    assert got == [0.0, 2.0 ** -9, 2.0 ** -9, 2.0 ** -6, 16.0, 20.0, 1.0, 1.25], got


def test_mirror_bf16_input_is_widened_exactly():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(5, 384, generator=g) * 3).bfloat16()
    q16, s16 = Q.quant_rows(x)
    q32, s32 = Q.quant_rows(x.float())
    assert torch.equal(q16.view(torch.uint8), q32.view(torch.uint8)) and torch.equal(s16, s32)
    dq = Q.dequant(q16, s16)
    # half an ulp of a 3-bit mantissa, half a subnormal step
    assert ((dq - x.float()).abs() <= 2.0 ** -4 * x.float().abs() + s16.unsqueeze(1) * 2.0 ** -10).all()
    # inv is 448 / amax, not 1 / scale: the two differ for some rows, and the mirror uses the former
    amax = x.float().abs().amax(dim=1)
    inv = torch.full_like(amax, 448.0) / amax
    assert torch.equal(q16.view(torch.uint8), (x.float() * inv.unsqueeze(1)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))


@pytest.mark.parametrize("tag", ["s", "xl"])
def test_fake_quant_oracle_distance_from_the_reference_golden(golden_dir, tag):
    """What W8A8 e4m3 with per-token / per-channel scales costs on these networks: E_q(tag), relative L2 on the O(1) output."""
    fx = torch.load(os.path.join(golden_dir, "dit_forward_b2.pt"), weights_only=True)
    cfg = CFGS[tag]
    sd = R.random_state_dict(cfg, seed=77)
    x = torch.randn((2, 4, 32, 32), generator=torch.Generator().manual_seed(501))
    cond = torch.zeros(2, 1000)
    cond[0, 417] = 1.0
    with torch.no_grad():
        out = Q.dit_forward_fq(sd, cfg, x, fx[f"{tag}/t"], cond)
    want = fx[f"{tag}/out"]
    rel, mx = float((out - want).norm() / want.norm()), float((out - want).abs().max())
    print(f"\n[fp8-ref] {tag}: rel {rel:.4f} max-abs {mx:.3f} (max |want| {float(want.abs().max()):.2f})")
    assert 0.03 <= rel <= 0.07, rel          # the lower bound: the oracle really quantises
    assert abs(rel - Q.E_Q[tag]) <= 0.05 * Q.E_Q[tag], (rel, Q.E_Q[tag])  # the constant the GPU tests use


def test_which_modules_take_the_mode(monkeypatch):
    from fastgen_amd import _lib
    from fastgen_amd.networks.DiT.network import DiT
    from fastgen_amd.networks.EDM.network import EDMPrecond
    from fastgen_amd.networks.EDM2.network import EDM2Precond

    edm_kw = dict(img_resolution=32, img_channels=3, label_dim=10, model_channels=128, channel_mult=[2, 2, 2])
    net = DiT(hidden_size=384, depth=1, num_heads=6, compute_dtype="fp8")
    assert net._select_dtype() == _lib.FG_DTYPE_FP8 == 3
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert DiT(hidden_size=384, depth=1, num_heads=6)._select_dtype() != _lib.FG_DTYPE_FP8   # never chosen by autocast
    with pytest.raises(ValueError, match="128"):
        DiT(hidden_size=384, depth=1, num_heads=6, mlp_ratio=3.5, compute_dtype="fp8")             # MLP width 1344 = 10.5 x 128
    with pytest.raises(ValueError, match="fp8"):
        EDMPrecond(compute_dtype="fp8", **edm_kw)
    with pytest.raises(ValueError, match="fp8"):
        EDM2Precond(img_resolution=16, img_channels=3, label_dim=0, model_channels=64, channel_mult=[1, 2], num_blocks=1,
                    attn_resolutions=[8], compute_dtype="fp8")
    monkeypatch.setenv("FASTGEN_AMD_COMPUTE_DTYPE", "fp8")
    assert DiT(hidden_size=384, depth=1, num_heads=6)._select_dtype() == _lib.FG_DTYPE_FP8
    monkeypatch.delenv("FASTGEN_AMD_COMPUTE_DTYPE")
    # the C ABI: a DiT handle in the mode; the U-Net handles refuse it
    L = _lib.lib()
    h = net._make_engine(_lib.FG_DTYPE_FP8)
    assert h.value
    L.fg_dit_destroy(h)
    cfg = _lib.fg_dit_config.from_buffer_copy(net._cfg)
    cfg.compute_dtype, cfg.mlp_hidden = _lib.FG_DTYPE_FP8, 1344
    h = ctypes.c_void_p()
    assert L.fg_dit_create(ctypes.byref(cfg), ctypes.byref(h)) == 1 and not h.value
    ecfg = _lib.fg_edm_config.from_buffer_copy(EDMPrecond(**edm_kw)._cfg)
    ecfg.compute_dtype = _lib.FG_DTYPE_FP8
    assert L.fg_edm_create(ctypes.byref(ecfg), ctypes.byref(h)) == 1 and b"compute_dtype" in L.fg_last_error()
    e2 = EDM2Precond(img_resolution=16, img_channels=3, label_dim=0, model_channels=64, channel_mult=[1, 2], num_blocks=1, attn_resolutions=[8])
    e2cfg = _lib.fg_edm2_config.from_buffer_copy(e2._cfg)
    e2cfg.compute_dtype = _lib.FG_DTYPE_FP8
    assert L.fg_edm2_create(ctypes.byref(e2cfg), ctypes.byref(h)) == 1 and b"compute_dtype" in L.fg_last_error()


def test_fp8_op_refusals():
    """fg_op_gemm_fp8 / fg_op_quant_rows_fp8 / fg_op_dit_ln_modulate_fp8 refuse what the kernels cannot run with FG_EINVAL before any
    launch (this runs without a GPU: the pointers are never dereferenced)."""
    from fastgen_amd import _lib

    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64)
    odd = ctypes.c_void_p(p.value + 4)

    def gemm(**kw):
        a = dict(a=p, w=p, bias=None, out=p, m=512, n=1152, k=1152, act=0, gate=None, gate_stride=0, gate_rows=256, resid=None,
                 tile_order=1, a_scale=p, w_scale=p)
        a.update(kw)
        return L.fg_op_gemm_fp8(*a.values(), None)

    for kw in (dict(k=1088), dict(k=64), dict(k=0), dict(n=1160), dict(n=8), dict(m=0), dict(act=2), dict(act=-1), dict(a=None),
               dict(w=None), dict(out=None), dict(a_scale=None), dict(w_scale=None), dict(w=odd), dict(w_scale=odd),
               dict(n=32768, k=65536), dict(tile_order=64), dict(gate=p, gate_stride=1148)):
        assert gemm(**kw) == 1, kw
        assert b"fg_op_gemm_fp8" in L.fg_last_error(), kw
    for args in ((0, p, p, p, 4, 192), (0, p, p, p, 0, 128), (2, p, p, p, 4, 128), (1, None, p, p, 4, 128), (1, p, p, None, 4, 128)):
        assert L.fg_op_quant_rows_fp8(*args, None) == 1, args
        assert b"fg_op_quant_rows_fp8" in L.fg_last_error()
    for d, ms, so in ((512, 2304, 0), (384, 2302, 0), (384, 2304, 2)):
        assert L.fg_op_dit_ln_modulate_fp8(p, p, ms, so, 384, p, p, 16, d, 256, None) == 1
        assert b"fg_op_dit_ln_modulate_fp8" in L.fg_last_error()
