"""`CausalWan(kv_cache_dtype="fp8")` on the GPU: the self-attention caches as e4m3 bytes + per-(token, head) scales through the cached calls.

A toy network (2 heads of 128, 2 layers, 5 frames of 16 x 24 latents = 96 tokens each, chunks of one frame, B 2, seeded random weights),
in both compute modes of the linears:
  - five cached autoregressive calls are finite, differ from the bf16-cache module's on the same weights (the path is taken) and stay
    within E_KV of them in relative L2.  MEASURED on an MI355X (first run of this file): 0.0037 with bf16 linears, 0.0134 with fp8
    linears (whose per-token e4m3 roundings a small change of the attention output moves; their own E_Q is 0.019 - 0.021); the bound
    is twice the measured value.
  - the fused student loop equals the per-call loop bit for bit, graph and eager, and a second video replays the same graphs;
  - cache_tag "neg" has its own e4m3 set: interleaved calls under the two tags give, per tag, the bits of a run under one tag alone;
  - the guided sampler runs on the e4m3 cache (graph == eager) - every cached entry point is covered, none refuses;
  - the setting cannot change once a cache set exists."""
import dataclasses

import pytest
import torch

from fastgen_amd import _lib

import test_wan as TW
from oracle import wan_ref as R

pytestmark = pytest.mark.gpu

KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2, chunk_size=1, total_num_frames=5, rope_max_seq_len=32)
E_KV_MEASURED = {"bf16": 0.00371, "fp8": 0.01338}  # per compute mode of the linears
MODES = ["bf16", "fp8"]


def _net(compute_dtype, kv):
    from fastgen_amd.networks.Wan.network_causal import CausalWan

    net = CausalWan(compute_dtype=compute_dtype, kv_cache_dtype=kv, **KW)
    net.load_state_dict(R.random_state_dict(dataclasses.replace(R.TINY, chunk_size=1, total_num_frames=5, rope_max_seq_len=32), 91), strict=True)
    return net.cuda().eval()


def _inputs(seed, B=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 16, 5, 16, 24, generator=g).cuda(), torch.randn(B, 16, 128, generator=g).cuda()


def _calls(net, x, text, tag="pos"):
    t = torch.full((x.shape[0],), 0.5, dtype=torch.float64, device="cuda")
    return [net(x[:, :, f: f + 1], t, condition=text, fwd_pred_type="flow", cache_tag=tag, cur_start_frame=f, store_kv=True, is_ar=True)
            for f in range(x.shape[2])]


@pytest.mark.parametrize("mode", MODES)
def test_cached_calls_stay_close_to_the_bf16_cache(mode):
    (x, text), net8, net16 = _inputs(92), _net(mode, "fp8"), _net(mode, None)
    with torch.inference_mode():
        got, want = torch.cat(_calls(net8, x, text), dim=2), torch.cat(_calls(net16, x, text), dim=2)
    assert torch.isfinite(got).all() and not torch.equal(got[:, :, 0], want[:, :, 0]) and not torch.equal(got, want)
    e = float((got - want).norm() / want.norm())
    print(f"\n[wan-kv8] compute_dtype {mode}: E_KV = rel-L2(fp8 cache, bf16 cache) = {e:.5f}")
    assert e <= 2 * E_KV_MEASURED[mode]


@pytest.mark.parametrize("mode", MODES)
def test_student_loop_graph_eager_and_per_call_agree_bit_for_bit(mode):
    net, net16 = _net(mode, "fp8"), _net(mode, "bf16")
    (lat, text), lat2 = _inputs(93), _inputs(94)[0]
    tl = torch.tensor([0.999, 0.6, 0.0], dtype=torch.float64, device="cuda")
    with torch.inference_mode():
        want = TW._per_call_loop(net, 0.999 * lat, tl, text, "ode")
        got = net.student_sample(0.999 * lat, tl, text, sample_type="ode")
        assert torch.isfinite(got).all() and torch.equal(got, want)
        assert torch.equal(net.student_sample(0.999 * lat, tl, text, sample_type="ode", use_graph=False), want)
        captures, launches = _lib.graph_stats()
        want2 = TW._per_call_loop(net, 0.999 * lat2, tl, text, "ode")
        assert torch.equal(net.student_sample(0.999 * lat2, tl, text, sample_type="ode"), want2)  # another video: the five chunk graphs again
        assert _lib.graph_stats() == (captures, launches + 5)
        assert not torch.equal(net16.student_sample(0.999 * lat, tl, text, sample_type="ode"), want)


def test_the_neg_tag_has_its_own_set_and_the_setting_is_fixed_once_allocated():
    (x, text), (xn, textn) = _inputs(95), _inputs(96)
    t = torch.full((2,), 0.5, dtype=torch.float64, device="cuda")
    net, alone_pos, alone_neg = (_net("bf16", "fp8") for _ in range(3))
    with torch.inference_mode():
        pos, neg = [], []
        for f in range(5):  # interleaved: a shared set would hand each tag the other's keys
            for outs, xx, tx, tag in ((pos, x, text, "pos"), (neg, xn, textn, "neg")):
                outs.append(net(xx[:, :, f: f + 1], t, condition=tx, fwd_pred_type="flow", cache_tag=tag, cur_start_frame=f, store_kv=True, is_ar=True))
        assert all(torch.equal(a, b) for a, b in zip(pos, _calls(alone_pos, x, text)))
        assert all(torch.equal(a, b) for a, b in zip(neg, _calls(alone_neg, xn, textn)))
    L = _lib.lib()
    assert L.fg_wan_set_kv_cache_dtype(net._h, _lib.FG_DTYPE_BF16) == 1 and b"kv_cache_dtype" in L.fg_last_error()
    assert L.fg_wan_set_kv_cache_dtype(net._h, _lib.FG_DTYPE_FP8) == 0  # (the setting it has)


def test_guided_sampler_runs_on_the_fp8_cache():
    noise, text = _inputs(97, B=1)
    kw = dict(condition=8.0 * text, neg_condition=-8.0 * text, guidance_scale=1.5, sample_steps=3)
    net, net16 = _net("bf16", "fp8"), _net("bf16", None)
    with torch.inference_mode():
        a = net.sample(noise.clone(), **kw)
        assert torch.isfinite(a).all() and torch.equal(net.sample(noise.clone(), use_graph=False, **kw), a)
        assert not torch.equal(net16.sample(noise.clone(), **kw), a)
