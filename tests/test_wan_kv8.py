"""The e4m3 self-attention cache of the causal video DiT (`CausalWan(kv_cache_dtype="fp8")`, fg_wan_set_kv_cache_dtype, the two ops of
fastgen_amd/csrc/wan_kv8.hip) without a device: the symbols, the argument refusals (made-up pointers: nothing is read before the checks are
through), the cache-size arithmetic and the keyword."""
import ctypes

import pytest

from fastgen_amd import _lib

KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2, chunk_size=1, total_num_frames=5)
P = [ctypes.c_void_p((i + 1) << 28) for i in range(6)]  # well separated, 16-byte aligned


def test_symbols_resolve_and_are_declared():
    for name in ("fg_wan_set_kv_cache_dtype", "fg_wan_kv_cache_bytes", "fg_op_wan_kv_quant", "fg_op_wan_attention_kv8"):
        assert name in _lib.SIGNATURES and getattr(_lib.lib(), name)


@pytest.mark.parametrize("kw", [dict(src=None), dict(k8=None), dict(scale=None), dict(heads=0), dict(heads=5), dict(rows=0), dict(rows=65), dict(l=0),
                                dict(start=-1), dict(start=37), dict(ld_src=255), dict(ld_src=257), dict(ld_dst=264), dict(ld_dst=128),
                                dict(dst_bs=100 * 256 + 16), dict(k8=ctypes.c_void_p((2 << 28) + 8)), dict(w=ctypes.c_void_p((3 << 28) + 4))])
def test_kv_quant_refuses(kw):
    a = dict(src=P[0], ld_src=768, w=P[1], eps=1e-6, cs=P[2], k8=P[3], scale=P[4], dst_bs=100 * 256, start=36, ld_dst=256, rows=128, l=64, heads=2, s=None)
    L = _lib.lib()
    assert L.fg_op_wan_kv_quant(*{**a, **kw}.values()) == 1 and b"fg_op_wan_kv_quant" in L.fg_last_error()


@pytest.mark.parametrize("kw", [dict(q=None), dict(v8=None), dict(ks=None), dict(out=None), dict(batch=0), dict(heads=0), dict(lq=0), dict(lkv=0),
                                dict(ldq=248), dict(ldq=260), dict(ldk=264), dict(ldk=128), dict(ldo=258), dict(q_bs=-8), dict(kv_bs=200 * 256 + 8),
                                dict(kv_bs=199 * 256), dict(scale_bs=399), dict(o_bs=95 * 256), dict(k8=ctypes.c_void_p((2 << 28) + 8))])
def test_attention_kv8_refuses(kw):
    a = dict(q=P[0], k8=P[1], v8=P[2], ks=P[3], vs=P[4], out=P[5], batch=2, heads=2, lq=96, lkv=200, ldq=256, ldk=256, ldo=256, q_bs=96 * 256,
             kv_bs=200 * 256, scale_bs=400, o_bs=96 * 256, s=None)
    L = _lib.lib()
    assert L.fg_op_wan_attention_kv8(*{**a, **kw}.values()) == 1 and b"fg_op_wan_attention_kv8" in L.fg_last_error()


def test_setter_refusals_and_cache_bytes():
    from fastgen_amd.networks.Wan.network_causal import CausalWan

    L = _lib.lib()
    net = CausalWan(**KW)
    assert L.fg_wan_set_kv_cache_dtype(None, _lib.FG_DTYPE_FP8) == 1
    for bad in (0, _lib.FG_DTYPE_F32, _lib.FG_DTYPE_BF16X3, 7):
        assert L.fg_wan_set_kv_cache_dtype(net._h, bad) == 1 and b"kv_cache_dtype" in L.fg_last_error()
    assert L.fg_wan_kv_cache_bytes(net._h, 0, 16, 24) == 0 and L.fg_wan_kv_cache_bytes(net._h, 1, 15, 24) == 0
    bf16 = net.kv_cache_bytes(3, 16, 24)
    assert bf16 == 2 * 2 * 3 * (5 * 8 * 12) * 256 * 2  # (K, V) x layers x batch x tokens x inner dim x 2 bytes
    fp8 = CausalWan(kv_cache_dtype="fp8", **KW).kv_cache_bytes(3, 16, 24)
    assert fp8 == bf16 // 2 + 2 * 2 * 3 * (5 * 8 * 12) * 2 * 4 and fp8 <= 0.53 * bf16
    assert L.fg_wan_set_kv_cache_dtype(net._h, _lib.FG_DTYPE_FP8) == 0 and net.kv_cache_bytes(3, 16, 24) == fp8  # (nothing allocated yet)


def test_keyword():
    from fastgen_amd.networks.Wan.network_causal import CausalWan

    with pytest.raises(ValueError, match="kv_cache_dtype"):
        CausalWan(kv_cache_dtype="int8", **KW)
    a, b = CausalWan(kv_cache_dtype=None, **KW), CausalWan(kv_cache_dtype="fp8", compute_dtype="fp8", **KW)
    assert a.kv_cache_dtype is None and b.kv_cache_dtype == "fp8" and list(a.state_dict()) == list(b.state_dict())
