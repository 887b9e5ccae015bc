"""CPU side of Wan2.2 TI2V-5B (fg_wan_create_ti2v, `WanI2V(concat_mask=False, ...)`, `Wan(expand_timesteps=True)`): the oracle of
tests/wan_ti2v_ref.py against itself and against tests/wan_full_ref.py, its mutants held apart, the module surface and the launch plans
of the 5B network's token GEMMs.

Mutant distances (relative L2 against the fp32 oracle on tests/wan_ti2v_ref.py's case, x0 prediction, video [2, 48, 5, 16, 24], t = 0.9;
frames >= 1 for the input-side mutants, the whole output for the others), measured on the CPU:
    no_input_replacement 0.149, first_frame_t_not_zero 0.328, no_output_replacement 0.508, neighbour_first_frame 0.129,
    convert_on_replaced_x_t 0.140
With R.random_state_dict as it is they are 0.011, 0.014, 0.570, 0.011, 0.286: the input-side ones below what a bf16 network's error lets a
test tell, hence the two scaled weight groups of `wan_ti2v_ref.random_state_dict`."""
import ctypes

import pytest
import torch

from fastgen_amd import _lib

import wan_full_ref as W
import wan_ti2v_ref as T
from oracle import wan_ref as R

FG_EINVAL, FG_ENOTREADY = 1, 2

TOL = 2e-2  # this network's tolerance in tests/test_gpu_wan_full.py
KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2)
TI2V = dict(concat_mask=False, use_image_encoder=False, expand_timesteps=True, image_dim=None, in_channels=48, out_channels=48)


def rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def case():
    return T.case()


def test_per_token_rows_equal_per_frame_rows(case):
    """What the engine relies on: the mask is constant within a latent frame, so one embedder row per token is one per frame."""
    sd, x, t, cond = case
    for i2v in (True, False):
        tok = T.WanTI2VRef(sd, T.TINY48, torch.float64, i2v=i2v).forward(x.double(), t, cond)
        frm = T.WanTI2VRef(sd, T.TINY48, torch.float64, i2v=i2v, per_frame_rows=True).forward(x.double(), t, cond)
        assert float((tok - frm).abs().max()) <= 1e-12 * float(tok.abs().max())


def test_t2v_with_expanded_timesteps_is_plain_wan(case):
    sd, x, t, cond = case
    got = T.WanTI2VRef(sd, T.TINY48, torch.float64, i2v=False).forward(x.double(), t, cond)
    want = W.WanFullRef(sd, T.TINY48, torch.float64).forward(x.double(), t, cond["text"])
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_mutants_are_apart(case):
    sd, x, t, cond = case
    want = T.WanTI2VRef(sd, T.TINY48).forward(x, t, cond, fwd_pred_type="x0")
    assert torch.equal(want[:, :, 0], cond["ff"][:, :, 0])
    for mu in T.MUTANTS:
        got = T.WanTI2VRef(sd, T.TINY48, mutant=mu).forward(x, t, cond, fwd_pred_type="x0")
        d = rel(got[:, :, 1:], want[:, :, 1:]) if mu in T.INPUT_SIDE else rel(got, want)
        print(mu, d)
        assert d >= 5 * TOL, (mu, d)


def test_loops_carry_the_first_frame(case):
    sd, x, t, cond = case
    net = T.WanTI2VRef(sd, T.TINY48)
    small = {"text": cond["text"], "ff": cond["ff"][..., :8, :8]}
    noise = x[..., :8, :8]
    tl = torch.tensor([0.999, 0.833, 0.0], dtype=torch.float64)
    for st in ("sde", "ode"):
        out = T.x0_loop(net, noise, tl, small, eps_list=[torch.ones_like(noise)], sample_type=st)
        assert torch.equal(out[:, :, 0], small["ff"][:, :, 0])
    neg = {"text": -cond["text"], "ff": small["ff"].flip(0)}
    out = T.guided_sample(net, noise, small, neg, 3.0, 2, solver="euler")
    assert torch.equal(out[:, :, 0], small["ff"][:, :, 0].double())


def _ti2v(**kw):
    from fastgen_amd.networks.WanI2V.network import WanI2V

    return WanI2V(**dict(dict(KW, **TI2V), **kw))


def test_state_dict_is_wans():
    from fastgen_amd.networks.Wan.network import Wan

    net = _ti2v()
    shapes = R.state_dict_shapes(T.TINY48)
    assert list(net.state_dict().keys()) == list(shapes)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == shapes
    plain = Wan(**KW, in_channels=48, out_channels=48, expand_timesteps=True)
    assert list(plain.state_dict().keys()) == list(shapes) and plain.expand_timesteps
    net.load_state_dict(T.random_state_dict(T.TINY48, 3), strict=True)
    plain.load_state_dict(T.random_state_dict(T.TINY48, 3), strict=True)
    assert net.is_i2v and net.is_ti2v and not net.concat_mask and not net.preserve_conditioning_is_identity
    assert net.fused_loop_preserves_conditioning
    assert net.supports_fused_loop("x0") and not net.supports_fused_loop("meanflow")


def test_preserve_conditioning_replaces_frame_0():
    net = _ti2v()
    x = torch.randn(2, 48, 3, 4, 4)
    for ff in (torch.randn(2, 48, 1, 4, 4), torch.randn(2, 48, 3, 4, 4)):
        y = net.preserve_conditioning(x, {"first_frame_cond": ff})
        assert y is not x and torch.equal(y[:, :, 0], ff[:, :, 0]) and torch.equal(y[:, :, 1:], x[:, :, 1:])
    assert net.preserve_conditioning(x, None) is x and net.preserve_conditioning(x, {"text_embeds": x}) is x


def test_refusals():
    from fastgen_amd.networks.Wan.network import Wan
    from fastgen_amd.networks.WanI2V.network import WanI2V

    # every mixture of the three flags but the two conventions
    for cm in (True, False):
        for ie in (True, False):
            for et in (True, False):
                if (cm and not et) or (cm, ie, et) == (False, False, True):
                    continue
                with pytest.raises(NotImplementedError, match=r"Wan2\.1 I2V.*Wan2\.2 TI2V"):
                    WanI2V(**dict(KW, concat_mask=cm, use_image_encoder=ie, expand_timesteps=et))
    with pytest.raises(ValueError, match="in_channels"):
        _ti2v(in_channels=36)
    with pytest.raises(ValueError, match="image_dim"):
        _ti2v(image_dim=1280)
    net = _ti2v()
    x, t = torch.zeros(1, 48, 2, 4, 4), torch.tensor([0.5])
    text = torch.zeros(1, 3, 128)
    with torch.no_grad():
        with pytest.raises(AssertionError, match="first_frame_cond"):
            net(x, t, condition={"text_embeds": text})
        with pytest.raises(AssertionError, match="must be a dict"):
            net(x, t, condition=text)
        with pytest.raises(RuntimeError, match="HIP GPU only"):
            net(x, t, condition={"text_embeds": text, "first_frame_cond": x[:, :, :1]})
    for bad in (torch.zeros(1, 48, 3, 4, 4), torch.zeros(1, 16, 1, 4, 4), torch.zeros(2, 48, 1, 4, 4), torch.zeros(1, 48, 1, 4, 6)):
        with pytest.raises(ValueError, match="first_frame_cond must be"):
            net._set_first_frame(bad, 1, 2, 4, 4, torch.device("cpu"))
    # t given per token, [B, seq_len], stays refused with a message that names [B] (the image-to-video network: tests/test_gpu_wan_ti2v.py)
    plain = Wan(**KW, in_channels=48, out_channels=48, expand_timesteps=True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r"t must be \[B\]"):
        plain(x, torch.zeros(1, 8), condition=text)


def test_c_abi_refusals():
    L = _lib.lib()
    assert ctypes.sizeof(_lib.fg_wan_ti2v_config) == 4

    def cfg(**kw):
        c = _lib.fg_wan_config()
        c.num_heads, c.head_dim, c.in_channels, c.out_channels, c.text_dim, c.freq_dim = 2, 128, 48, 48, 128, 256
        c.ffn_dim, c.num_layers, c.rope_max_seq_len, c.chunk_size, c.total_num_frames, c.eps = 512, 1, 64, 1, 1, 1e-6
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    t = _lib.fg_wan_ti2v_config()
    t.latent_channels = 48
    h = ctypes.c_void_p()
    for bad in (cfg(in_channels=36), cfg(out_channels=16)):
        assert L.fg_wan_create_ti2v(ctypes.byref(bad), None, ctypes.byref(t), ctypes.byref(h)) == FG_EINVAL and b"latent_channels" in L.fg_last_error()
    assert L.fg_wan_create_ti2v(ctypes.byref(cfg()), None, None, ctypes.byref(h)) == FG_EINVAL
    # the 5B width is a width of the engine now; 3200 is not
    assert L.fg_wan_create_ti2v(ctypes.byref(cfg(num_heads=25)), None, ctypes.byref(t), ctypes.byref(h)) == FG_EINVAL and b"3072" in L.fg_last_error()
    assert L.fg_wan_create_ti2v(ctypes.byref(cfg(num_heads=24, ffn_dim=14336)), None, ctypes.byref(t), ctypes.byref(h)) == 0
    L.fg_wan_destroy(h)
    assert L.fg_wan_create_ti2v(ctypes.byref(cfg()), None, ctypes.byref(t), ctypes.byref(h)) == 0
    plain = ctypes.c_void_p()
    assert L.fg_wan_create(ctypes.byref(cfg()), ctypes.byref(plain)) == 0
    try:
        assert L.fg_wan_num_params(h) == L.fg_wan_num_params(plain)
        fake = ctypes.c_void_p(256)
        assert L.fg_wan_set_first_frame(plain, fake, 1, 4, 4, None) == FG_EINVAL and b"fg_wan_create_ti2v" in L.fg_last_error()
        assert L.fg_wan_set_first_frame(h, fake, 1, 3, 4, None) == FG_EINVAL
        assert L.fg_wan_set_first_frame(h, None, 1, 4, 4, None) == FG_EINVAL
        assert L.fg_wan_first_frame_read(h, fake, None) == FG_ENOTREADY
        assert L.fg_wan_first_frame_read(plain, fake, None) == FG_EINVAL
        # the chunked and causal entry points
        assert L.fg_wan_forward(h, fake, fake, ctypes.c_void_p(512), 1, 1, 4, 4, 0, 0, fake, 1 << 30, None) == FG_EINVAL
        assert b"image-to-video" in L.fg_last_error()
        assert L.fg_wan_forward_block_causal(h, fake, fake, ctypes.c_void_p(512), 1, 1, 4, 4, fake, 1 << 30, None) == FG_EINVAL
        # the op entry points refuse before they launch
        assert L.fg_op_wan_patch_embed(fake, None, fake, fake, fake, 1, 16, 1, 4, 4, 256, 2, None) == FG_EINVAL
        assert L.fg_op_wan_patch_embed(fake, None, fake, fake, fake, 1, 48, 1, 4, 5, 256, 0, None) == FG_EINVAL
        assert L.fg_op_wan_final(fake, fake, fake, fake, None, fake, 1, 16, 1, 2, 2, 256, 1e-6, 2, None) == FG_EINVAL
        assert L.fg_op_wan_final(fake, fake, fake, fake, None, fake, 1, 48, 1, 2, 2, 320, 1e-6, 1, None) == FG_EINVAL
    finally:
        L.fg_wan_destroy(h)
        L.fg_wan_destroy(plain)


@pytest.mark.parametrize("keeps", [True, False])
def test_generator_fn_and_the_hook(monkeypatch, keeps):
    """A network whose fused loop restates its `preserve_conditioning` hook keeps the fused loop; without the attribute a real hook
    sends generator_fn to the generic loop."""
    from fastgen_amd.methods.model import FastGenModel

    net = _ti2v()
    net.fused_loop_preserves_conditioning = keeps
    seen = {}

    def few_step_sample(noise, condition, t_list, **kw):
        seen.update(fused=True, steps=len(t_list) - 1)
        return noise.clone()

    def generic(cls_net, x, t_list, **kw):
        seen.update(generic=True)
        return x

    monkeypatch.setattr(net, "few_step_sample", few_step_sample)
    cond = {"text_embeds": torch.zeros(1, 3, 128), "first_frame_cond": torch.zeros(1, 48, 1, 4, 4)}
    noise = torch.ones(1, 48, 2, 4, 4)
    if keeps:
        FastGenModel.generator_fn(net, noise, student_sample_steps=2, condition=cond)
        assert seen == {"fused": True, "steps": 2}
    else:
        with pytest.raises(RuntimeError, match="HIP GPU only"):  # (the generic loop calls the network, which needs a GPU)
            FastGenModel.generator_fn(net, noise, student_sample_steps=2, condition=cond)
        assert not seen


def test_gemm_plans_of_the_5b_network():
    """The five (N, K) pairs of a 5B block - qkv 9216 x 3072, the D x D linears, kv 6144 x 3072, the two feed-forward ones - through the
    launch plan at the 5B shape's 18 480 tokens (880 per frame: the gate period) and at one short sample, in bf16 and fp8."""
    import test_gemm_plan as G

    for fl in (G.BF16, G.FP8):
        for n, k in ((9216, 3072), (3072, 3072), (6144, 3072), (14336, 3072), (3072, 14336)):
            for m, gate_rows in ((18480, 880), (18480, 0), (480, 96), (36960, 880)):
                for scratch in (0, 16 * m * 3072):
                    p = dict(zip(G.FIELDS, G.plan(fl, m, n, k, gate_rows=gate_rows, scratch=scratch)))
                    assert p["refusal"] == 0, (fl, m, n, k, p)
                    assert not G.violations(fl, m, n, k, 0, gate_rows, scratch, 1, 0, 256), (fl, m, n, k)
