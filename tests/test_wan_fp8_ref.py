"""The fp8 (e4m3fn, W8A8) compute mode of the causal video DiT without a GPU: how far the quantisation itself moves the network (the
fake-quant oracle of tests/wan_fp8_ref.py against the plain oracle, both fp64: E_Q, the yardstick of tests/test_gpu_wan_fp8.py), that
the four mutant schemes are far enough from the stated one to be told apart, and what the module and the C ABI accept."""
import ctypes

import pytest
import torch

import wan_fp8_ref as W
from oracle import wan_ref as R

KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2, chunk_size=2, total_num_frames=6)
FG_EINVAL = 1


@pytest.mark.parametrize("tag", list(W.CONFIGS))
def test_fake_quant_oracle_distance_from_the_plain_oracle(tag):
    """E_Q(tag, call): what W8A8 e4m3 with per-token / per-channel scales on the six block linears costs, relative L2 of the output."""
    plain, fq = W.oracle_outputs(tag, "plain"), W.oracle_outputs(tag, "fq")
    for call in W.CALLS:
        e = W.rel(fq[call], plain[call])
        print(f"\n[wan-fp8-ref] {tag} {call}: E_Q {e:.5f} (constant {W.E_Q[tag][call]})")
        assert plain[call].dtype == fq[call].dtype == torch.float64
        assert 0.01 <= e <= 0.04, e  # the lower bound: the oracle really quantises
        assert abs(e - W.E_Q[tag][call]) <= 0.05 * W.E_Q[tag][call], (tag, call, e)  # the constant the GPU tests use


@pytest.mark.parametrize("tag", list(W.CONFIGS))
def test_every_mutant_is_far_from_the_fake_quant_oracle(tag):
    """The GPU test tells the stated scheme from a mutant by which oracle the output is closer to; that needs each mutant's own distance
    from the fake-quant oracle to be well above nothing: > 0.1 E_Q on every call (measured on these seeded inputs: `no_ffn2` 0.48 - 0.50,
    `per_tensor_act` 0.95 - 1.00, `weights_unquantised` 1.01 - 1.04, `amax_240` 1.37 - 1.47 E_Q - no other inputs were needed)."""
    fq = W.oracle_outputs(tag, "fq")
    for m in W.MUTANTS:
        out = W.oracle_outputs(tag, m)
        for call in W.CALLS:
            d = W.rel(out[call], fq[call])
            print(f"\n[wan-fp8-ref] {tag} {call} mutant {m}: {d:.5f} = {d / W.E_Q[tag][call]:.3f} E_Q")
            assert d > 0.1 * W.E_Q[tag][call], (tag, m, call, d)


def test_the_oracle_swaps_the_six_block_linears_and_nothing_else():
    seen = []
    plain = R._lin
    p = {n + s: torch.zeros(4, 128) if s == ".weight" else torch.zeros(4) for n in
         ["blocks.0." + l for l in W.FP8_LINEARS + ("attn2.to_k", "attn2.to_v")] + ["proj_out", "condition_embedder.time_proj"] for s in (".weight", ".bias")}
    x = torch.randn(3, 128, generator=torch.Generator().manual_seed(1))
    with W.fake_quant_oracle():
        assert R._lin is not plain
        for name in sorted({k.rsplit(".", 1)[0] for k in p}):
            q = dict(p)
            q[name + ".weight"] = torch.eye(128)[:4] * 1.0
            got = R._lin(q, x, name)
            if not torch.equal(got, x[:, :4]):  # (an identity weight is exact in e4m3: only the quantised activation moves the result)
                seen.append(name[len("blocks.0."):])
    assert R._lin is plain  # restored
    assert sorted(seen) == sorted(W.FP8_LINEARS), seen


def test_module_takes_the_mode():
    from fastgen_amd.networks.Wan.network_causal import CausalWan

    net16, net8 = CausalWan(**KW), CausalWan(compute_dtype="fp8", **KW)
    assert net16.compute_dtype is None and net8.compute_dtype == "fp8" and CausalWan(compute_dtype="bf16", **KW).compute_dtype == "bf16"
    a, b = net16.state_dict(), net8.state_dict()
    assert list(a) == list(b) == list(R.state_dict_shapes(R.TINY))  # the same key list: fp32 masters, nothing packed in the state dict
    assert all(a[k].shape == b[k].shape and b[k].dtype == torch.float32 for k in a)
    for bad in ("fp32", "bf16x3"):
        with pytest.raises(ValueError, match="compute_dtype"):
            CausalWan(compute_dtype=bad, **KW)
    with pytest.raises(TypeError):
        CausalWan(2, 128, 16, 16, 128, 256, 512, 2, 1e-6, 1024, False, "flow", "rf", 2, 6, True, "fp8")  # keyword only
    # ffn_dim 576 = 4.5 x 128: the K of ffn.net.2 is no multiple of the e4m3 MFMA's K-step
    with pytest.raises(ValueError, match="128"):
        CausalWan(compute_dtype="fp8", **dict(KW, ffn_dim=576))
    CausalWan(**dict(KW, ffn_dim=576))
    CausalWan(compute_dtype="bf16", **dict(KW, ffn_dim=576))


def _abi_cfg(**kw):
    from fastgen_amd import _lib

    cfg = _lib.fg_wan_config()
    cfg.num_heads, cfg.head_dim, cfg.in_channels, cfg.out_channels, cfg.text_dim, cfg.freq_dim = 2, 128, 16, 16, 128, 256
    cfg.ffn_dim, cfg.num_layers, cfg.rope_max_seq_len, cfg.chunk_size, cfg.total_num_frames, cfg.eps = 512, 2, 1024, 2, 6, 1e-6
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_abi_compute_dtype():
    """fg_wan_create: 0 (a zero-initialised struct) and FG_DTYPE_BF16 are the bf16 mode, FG_DTYPE_FP8 the fp8 mode, anything else
    FG_EINVAL naming the field; fp8 refuses ffn_dim % 128 != 0; a bf16 handle's workspace is what it was, an fp8 handle's grows by the
    quantised operands.  No device call: this runs without a GPU."""
    from fastgen_amd import _lib

    L = _lib.lib()
    assert ctypes.sizeof(_lib.fg_wan_config) == 13 * 4 and _lib.fg_wan_config.compute_dtype.offset == 12 * 4  # the new field trails

    def create(**kw):
        h = ctypes.c_void_p()
        rc = L.fg_wan_create(ctypes.byref(_abi_cfg(**kw)), ctypes.byref(h))
        return rc, h

    handles = {}
    for name, dt in (("unset", 0), ("bf16", _lib.FG_DTYPE_BF16), ("fp8", _lib.FG_DTYPE_FP8)):
        rc, h = create(compute_dtype=dt)
        assert rc == 0 and h.value, name
        handles[name] = h
    try:
        for dt in (7, _lib.FG_DTYPE_BF16X3, -1):
            rc, h = create(compute_dtype=dt)
            assert rc == FG_EINVAL and not h.value and b"compute_dtype" in L.fg_last_error(), dt
        rc, h = create(compute_dtype=_lib.FG_DTYPE_FP8, ffn_dim=576)
        assert rc == FG_EINVAL and not h.value and b"ffn_dim" in L.fg_last_error()
        rc, h = create(compute_dtype=_lib.FG_DTYPE_BF16, ffn_dim=576)
        assert rc == 0 and h.value
        L.fg_wan_destroy(h)
        # workspace: B 1, 2 frames of 16 x 16 latents = 128 tokens; the fp8 plan adds [M][D] + [M][ffn] bytes and two [M] fp32 scale
        # vectors (each rounded up to 256 bytes) behind the bf16 plan
        ws = {k: L.fg_wan_workspace_bytes(h, 1, 2, 16, 16) for k, h in handles.items()}
        assert ws["unset"] == ws["bf16"] > 0
        M = 128
        assert ws["fp8"] == ws["bf16"] + M * 256 + M * 512 + 2 * 512, ws
        assert all(L.fg_wan_num_params(h) == L.fg_wan_num_params(handles["bf16"]) for h in handles.values())
    finally:
        for h in handles.values():
            L.fg_wan_destroy(h)


def test_ln_modulate_fp8_op_still_refuses_what_it_cannot_run():
    """fg_op_dit_ln_modulate_fp8 takes the video DiT's widths now; d = 512 and misaligned strides / offsets are still FG_EINVAL before
    any launch (the pointers are never dereferenced)."""
    from fastgen_amd import _lib

    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64)
    for d, ms, so, co in ((512, 3072, 0, 512), (640, 3840, 0, 640), (256, 1534, 0, 256), (1536, 9216, 2, 1536), (5120, 30720, 0, 5122),
                          (2048, 12288, -4, 2048)):
        assert L.fg_op_dit_ln_modulate_fp8(p, p, ms, so, co, p, p, 16, d, 64, None) == FG_EINVAL, (d, ms, so, co)
        assert b"fg_op_dit_ln_modulate_fp8" in L.fg_last_error()
    assert L.fg_op_dit_ln_modulate_fp8(None, p, 1536, 0, 256, p, p, 16, 256, 64, None) == FG_EINVAL
    assert L.fg_op_dit_ln_modulate_fp8(p, p, 1536, 0, 256, p, p, 0, 256, 64, None) == FG_EINVAL
