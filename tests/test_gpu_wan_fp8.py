"""The causal video DiT in the fp8 compute mode (`CausalWan(compute_dtype="fp8")`, fg_wan_config.compute_dtype = FG_DTYPE_FP8: the six
block linears that read the video tokens on e4m3fn operands, everything else as in the bf16 mode) on the GPU.

Two configurations (tests/wan_fp8_ref.py CONFIGS, B 1, two layers, seeded random weights - the network's parity is unpinned):
  "reg"  inner dim 256, ffn 512, 64 tokens per frame: every GEMM on the register-staged kernel (M = 128, and 384 in the block-causal call)
  "pp"   inner dim 384, ffn 1024, 256 tokens per frame, chunks of 2 frames: M = 512, gate_rows = 256 - the smallest shape at which the
         ping-pong kernel and its two-gate-row token epilogue run (the block-causal call: M = 1024)
and three calls each: chunk 0 with store_kv, chunk 1 over that cache, the block-causal call over all frames with per-frame timesteps.
Against the fp64 oracles of tests/wan_fp8_ref.py, with E_Q = rel-L2(fake-quant oracle, plain oracle) pinned by tests/test_wan_fp8_ref.py:
  (a) rel-L2(fp8 output, PLAIN oracle) <= 2 E_Q - the factor tests/test_gpu_dit_fp8.py gives the DiT, for the same reason: the kernels
      keep bf16 tensors between the linears (attention outputs, the GELU hidden, the stream), which moves roundings of the e4m3 operands;
  (b) the output is closer to the fake-quant oracle than to EACH mutant oracle (activations scaled per tensor, weights unquantised,
      ffn.net.2 left out, amax / 240): parameter-free - an engine that follows a mutant's scheme is closer to that mutant;
  (c) rel-L2(fp8 output, bf16 module's output on the same weights) > 0.25 E_Q: the fp8 path was taken.
MEASURED on an MI355X (first run of this file; the six cases): (a) 1.02 - 1.06 E_Q; (b) d(fp8, fq) 0.0126 - 0.0142 against the nearest
mutant's (`no_ffn2`) 0.0131 - 0.0148, the others 0.019 - 0.031; (c) 1.02 - 1.06 E_Q, the bf16 mode itself at 0.0042 - 0.0045 of the oracle.

The quantising LayerNorm-modulate at the video DiT's widths: the method and bound of tests/test_gpu_gemm_fp8.py::test_ln_modulate_fp8."""
import ctypes

import pytest
import torch

from fastgen_amd import _lib

import test_wan as TW
import wan_fp8_ref as W
from oracle import wan_ref as R

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _module(cfg, sd, compute_dtype):
    from fastgen_amd.networks.Wan.network_causal import CausalWan

    net = CausalWan(num_attention_heads=cfg.num_heads, attention_head_dim=cfg.head_dim, text_dim=cfg.text_dim, ffn_dim=cfg.ffn_dim,
                    num_layers=cfg.num_layers, chunk_size=cfg.chunk_size, total_num_frames=cfg.total_num_frames, compute_dtype=compute_dtype)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


@pytest.mark.parametrize("d", [256, 1536, 2048, 5120])
def test_ln_modulate_fp8_at_the_video_widths(d):
    from fastgen_amd import _lib

    ntok, tpi = 300, 96  # a modulation row per 96 tokens (four rows, the last one short); a ragged last workgroup (16 tokens each)
    g = torch.Generator().manual_seed(d)
    x = (torch.randn(ntok, d, generator=g) * 2 + 0.3 * torch.randn(ntok, 1, generator=g)).bfloat16()
    mod = 0.5 * torch.randn(4, 6 * d, generator=g)
    shift_off, scale_off = 3 * d, 4 * d
    xd, md = x.cuda(), mod.cuda()
    y8 = torch.full((ntok + 16, d), 0x55, dtype=torch.uint8, device="cuda")  # (16 guard rows behind the last token)
    ys = torch.full((ntok + 16,), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().fg_op_dit_ln_modulate_fp8(_p(xd), _p(md), 6 * d, shift_off, scale_off, _p(y8), _p(ys), ntok, d, tpi,
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert bool((y8[ntok:] == 0x55).all()) and bool((ys[ntok:] == -7.0).all())  # nothing written behind the last token
    y8, ys = y8[:ntok], ys[:ntok]
    x64, m64 = x.double(), mod.double().repeat_interleave(tpi, dim=0)[:ntok]
    y = torch.nn.functional.layer_norm(x64, (d,), eps=1e-6) * (1 + m64[:, scale_off: scale_off + d]) + m64[:, shift_off: shift_off + d]
    amax = y.abs().amax(dim=1)
    scale = ys.cpu().double()
    ulp = (scale.float().abs().frexp().exponent.double() - 24).exp2()  # fp32 ulp at the scale's binade
    worst = float(((scale - amax / 448.0).abs() / ulp).max())
    deq = y8.cpu().view(torch.float8_e4m3fn).double() * scale.unsqueeze(1)
    bound = 2.0 ** -4 * y.abs() + scale.unsqueeze(1) * 2.0 ** -10 + 1e-5 * amax.unsqueeze(1)
    print(f"\n[wan-ln-fp8] d {d}: scale off by {worst:.2f} ulp at most; max (|deq - y| / bound) {float(((deq - y).abs() / bound).max()):.3f}")
    assert worst <= 4.0, worst
    assert ((deq - y).abs() <= bound).all()


def _module_calls(net, tag):
    def forward(x, t, text, start, store, bc):
        return net(x.cuda(), t.cuda(), condition=text.cuda(), fwd_pred_type="flow", cur_start_frame=start, store_kv=store, is_ar=not bc).cpu()

    with torch.inference_mode():
        out = W.run_calls(tag, forward)
        net.clear_caches()
    return out


@pytest.mark.parametrize("tag", list(W.CONFIGS))
def test_forward_against_the_oracles(tag):
    cfg, sd, _, _, _ = W.case(tag)
    got = _module_calls(_module(cfg, sd, "fp8"), tag)
    got16 = _module_calls(_module(cfg, sd, "bf16"), tag)
    plain, fq = W.oracle_outputs(tag, "plain"), W.oracle_outputs(tag, "fq")
    mutants = {m: W.oracle_outputs(tag, m) for m in W.MUTANTS}
    fails = []
    for call in W.CALLS:
        o, e = got[call], W.E_Q[tag][call]
        assert o.shape == plain[call].shape and torch.isfinite(o).all()
        d_plain, d_fq, d_16 = W.rel(o, plain[call]), W.rel(o, fq[call]), W.rel(o, got16[call])
        d_mut = {m: W.rel(o, mutants[m][call]) for m in W.MUTANTS}
        print(f"\n[wan-fp8] {tag} {call}: E_Q {e:.4f}  d(fp8, plain) {d_plain:.4f} = {d_plain / e:.2f} E_Q   d(fp8, fq) {d_fq:.4f}   "
              f"d(fp8, bf16 mode) {d_16:.4f} = {d_16 / e:.2f} E_Q   d(bf16 mode, plain) {W.rel(got16[call], plain[call]):.4f}   d(fp8, mutant) "
              + "  ".join(f"{m} {v:.4f}" for m, v in d_mut.items()))
        if not d_plain <= 2 * e:
            fails.append(("a", call, d_plain, e))
        fails += [("b", call, m, d_fq, v) for m, v in d_mut.items() if not d_fq < v]
        if not d_16 > 0.25 * e:
            fails.append(("c", call, d_16, e))
    assert not fails, fails


def _toy(seed, compute_dtype="fp8"):
    """The toy shape of tests/test_wan.py: TINY, 5 frames (chunks of 3 + 2), 16 x 16 latents."""
    sd = R.random_state_dict(R.TINY, seed)
    net = _module(R.TINY, sd, compute_dtype)
    g = torch.Generator().manual_seed(seed + 1)
    lat = torch.randn(1, 16, 5, 16, 16, generator=g).cuda()
    text = torch.randn(1, 16, 128, generator=g).cuda()
    return net, sd, lat, text


def test_student_loop_graph_eager_and_per_call_agree_bit_for_bit():
    net, _, lat, text = _toy(71)
    net16 = _toy(71, "bf16")[0]
    lat = lat * 0.999
    tl = torch.tensor([0.999, 0.7, 0.3, 0.0], dtype=torch.float64, device="cuda")
    with torch.inference_mode():
        want = TW._per_call_loop(net, lat.clone(), tl, text, "ode")
        got = net.student_sample(lat.clone(), tl, text, sample_type="ode")
        assert torch.isfinite(got).all() and torch.equal(got, want)
        captures, launches = _lib.graph_stats()
        assert torch.equal(net.student_sample(lat.clone(), tl, text, sample_type="ode"), want)  # replay of the cached chunk graphs
        assert _lib.graph_stats() == (captures, launches + 2)
        assert torch.equal(net.student_sample(lat.clone(), tl, text, sample_type="ode", use_graph=False), want)
        # ... and it is the fp8 arithmetic that ran: the bf16 module on the same weights gives another video
        assert not torch.equal(net16.student_sample(lat.clone(), tl, text, sample_type="ode"), want)


def test_guided_sampler_graph_and_eager_agree_bit_for_bit():
    net, _, noise, text = _toy(73)
    net16 = _toy(73, "bf16")[0]
    kw = dict(condition=8.0 * text, neg_condition=-8.0 * text, guidance_scale=1.5, sample_steps=3)
    with torch.inference_mode():
        a = net.sample(noise.clone(), **kw)
        assert torch.isfinite(a).all()
        captures, launches = _lib.graph_stats()
        assert torch.equal(net.sample(noise.clone(), **kw), a)  # the cached graphs
        assert _lib.graph_stats() == (captures, launches + 2)
        assert torch.equal(net.sample(noise.clone(), use_graph=False, **kw), a)
        assert not torch.equal(net16.sample(noise.clone(), **kw), a)


def test_feature_taps_run_in_the_mode_and_leave_the_output_alone():
    """fg_wan_forward_features on an fp8 handle, every block tapped: the same output bits as fg_wan_forward, finite taps, and the taps
    are the fp8 stream's (the last block's x_ffn differs from the bf16 handle's)."""
    from fastgen_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda:0")
    cfg, sd, x, text, _ = W.case("reg")
    Fr, hw, D, depth = cfg.chunk_size, x.shape[-1], cfg.dim, cfg.num_layers
    Ltok = Fr * (hw // 2) ** 2
    xd, td, textd = x[:, :, :Fr].contiguous().to(dev), torch.full((1, Fr), 300.0, device=dev), text.to(dev).contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    last = {}
    for mode in ("fp8", "bf16"):
        net = _module(cfg, sd, mode)
        net._bind(dev)
        ws = torch.empty(L.fg_wan_workspace_bytes(net._h, 1, Fr, hw, hw), dtype=torch.uint8, device=dev)
        _lib.check(L.fg_wan_set_text(net._h, _p(textd), 1, textd.shape[1], _p(ws), ws.numel(), stream))
        plain, out = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
        _lib.check(L.fg_wan_forward(net._h, _p(xd), _p(td), _p(plain), 1, Fr, hw, hw, 0, 0, _p(ws), ws.numel(), stream))
        blocks = [{k: torch.full((1, Ltok, D), float("nan"), device=dev) for k in ("attn1", "x_attn1", "attn2", "x_attn2", "x_ffn")} for _ in range(depth)]
        taps = (_lib.fg_wan_block_taps * depth)()
        for i, b in enumerate(blocks):
            for k, v in b.items():
                setattr(taps[i], k, v.data_ptr())
        tokens, temb = torch.full((1, Ltok, D), float("nan"), device=dev), torch.full((Fr, D), float("nan"), device=dev)
        _lib.check(L.fg_wan_forward_features(net._h, _p(xd), _p(td), _p(out), 1, Fr, hw, hw, 0, 0, 0, (ctypes.c_int * depth)(*range(depth)), taps,
                                             depth, _p(tokens), _p(temb), _p(ws), ws.numel(), stream))
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and torch.equal(out, plain), mode
        assert all(torch.isfinite(v).all() for b in blocks for v in b.values()) and torch.isfinite(tokens).all() and torch.isfinite(temb).all()
        last[mode] = blocks[-1]["x_ffn"].cpu()
    assert not torch.equal(last["fp8"], last["bf16"])


def _one_call(net, lat, text):
    t = torch.full((1,), 0.5, dtype=torch.float64, device="cuda")
    with torch.inference_mode():
        out = net(lat[:, :, :2], t, condition=text, fwd_pred_type="flow", cur_start_frame=0, store_kv=True, is_ar=True)
        net.clear_caches()
    return out


def test_default_is_the_bf16_mode_bit_for_bit():
    net, sd, lat, text = _toy(75, None)
    assert torch.equal(_one_call(net, lat, text), _one_call(_module(R.TINY, sd, "bf16"), lat, text))


def test_a_weight_update_requantises():
    net, _, lat, text = _toy(77)
    before = _one_call(net, lat, text)
    with torch.no_grad():
        net.get_parameter("transformer.blocks.1.ffn.net.2.weight").mul_(1.25)
    fresh = _module(R.TINY, {k: v.cpu() for k, v in net.state_dict().items()}, "fp8")
    after = _one_call(net, lat, text)
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    assert torch.equal(_one_call(fresh, lat, text), after)
