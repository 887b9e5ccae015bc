"""CPU side of the image-to-video network (fg_wan_create_i2v, fastgen_amd.networks.WanI2V): the parameter table against
tests/wan_i2v_ref.py, the refusals the C ABI makes from its arguments alone, the mask algebra, the distance of the oracle's mutants on
the inputs the GPU forward test uses, and the module's surface.  Nothing here touches a GPU."""
import ctypes
import functools

import pytest
import torch

from oracle import wan_ref as R
import wan_i2v_ref as I

FG_EINVAL, FG_ENOTREADY = 1, 2
TOL, MUTANT_FACTOR = 2e-2, 5.0  # tests/test_gpu_wan_i2v.py's forward tolerance; the project's factor (tests/test_gpu_wan_blocks.py)
KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _cfg(in_channels=36, out_channels=16):
    from fastgen_amd import _lib

    c = _lib.fg_wan_config()
    c.num_heads, c.head_dim, c.in_channels, c.out_channels, c.text_dim, c.freq_dim = 2, 128, in_channels, out_channels, 128, 256
    c.ffn_dim, c.num_layers, c.rope_max_seq_len, c.chunk_size, c.total_num_frames, c.eps = 512, 2, 1024, 1, 1, 1e-6
    return c


def _i2v(latent=16, mask=4, image_dim=128):
    from fastgen_amd import _lib

    v = _lib.fg_wan_i2v_config()
    v.latent_channels, v.mask_channels, v.image_dim = latent, mask, image_dim
    return v


def _table(L, h):
    name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 5)()
    out = []
    for i in range(L.fg_wan_num_params(h)):
        assert L.fg_wan_param_info(h, i, ctypes.byref(name), ctypes.byref(ndim), shape) == 0
        out.append((name.value.decode(), tuple(shape[j] for j in range(ndim.value))))
    return out


def test_table_and_refusals_without_a_gpu():
    from fastgen_amd import _lib

    L = _lib.lib()
    assert ctypes.sizeof(_lib.fg_wan_i2v_config) == 3 * 4
    made = []

    def create(cfg, i2v):
        h = ctypes.c_void_p()
        rc = L.fg_wan_create_i2v(ctypes.byref(cfg), None, ctypes.byref(i2v), ctypes.byref(h))
        if rc == 0:
            made.append(h)
        return rc, h

    try:
        # ---- the table: the reference shapes in order; insertions only at the two named places
        rc, h = create(_cfg(), _i2v())
        assert rc == 0
        tab = _table(L, h)
        want = I.state_dict_shapes(I.TINY, 128)
        assert [n for n, _ in tab] == list(want) and dict(tab) == want
        plain = ctypes.c_void_p()
        assert L.fg_wan_create_ex(ctypes.byref(_cfg()), None, ctypes.byref(plain)) == 0
        made.append(plain)
        base = _table(L, plain)
        assert [e for e in tab if e in base] == base and len(tab) == len(base) + 8 + 5 * 2
        names = [n for n, _ in tab]
        at = names.index("transformer.condition_embedder.text_embedder.linear_2.bias")
        assert names[at + 1: at + 9] == [I.IMG_EMB + k for k in I.IMG_EMB_KEYS]
        for i in range(2):
            at = names.index(f"transformer.blocks.{i}.attn2.norm_k.weight")
            assert names[at + 1: at + 6] == [f"transformer.blocks.{i}." + k for k in I.IMG_BLK_KEYS]
        rc, h0 = create(_cfg(), _i2v(image_dim=0))
        assert rc == 0 and _table(L, h0) == base

        # ---- creation refusals, each naming its field
        for cfg, i2v, word in ((_cfg(in_channels=35), _i2v(), b"in_channels"), (_cfg(out_channels=8), _i2v(), b"out_channels"),
                               (_cfg(), _i2v(mask=1), b"mask_channels"), (_cfg(in_channels=33), _i2v(mask=1), b"mask_channels"),
                               (_cfg(), _i2v(image_dim=100), b"image_dim"), (_cfg(), _i2v(image_dim=-64), b"image_dim")):
            rc, hb = create(cfg, i2v)
            assert rc == FG_EINVAL and not hb.value and word in L.fg_last_error(), word
        hb = ctypes.c_void_p()
        assert L.fg_wan_create_i2v(ctypes.byref(_cfg()), None, None, ctypes.byref(hb)) == FG_EINVAL

        # ---- the chunked / causal entry points on an image-to-video handle
        fake, out = ctypes.c_void_p(4096), ctypes.c_void_p(8192)  # non-null, 256-byte aligned, never dereferenced
        word = b"not implemented for an image-to-video handle"
        assert L.fg_wan_forward(h, fake, fake, out, 1, 1, 16, 16, 0, 0, fake, 1 << 30, None) == FG_EINVAL and word in L.fg_last_error()
        assert L.fg_wan_forward_block_causal(h, fake, fake, out, 1, 1, 16, 16, fake, 1 << 30, None) == FG_EINVAL and word in L.fg_last_error()
        for bc in (0, 1):
            assert L.fg_wan_forward_features(h, fake, fake, out, 1, 1, 16, 16, 0, 0, bc, None, None, 0, None, None, fake, 1 << 30,
                                             None) == FG_EINVAL and word in L.fg_last_error()
        sc = _lib.fg_wan_sampler_config()
        sc.t_scale, sc.net_pred_flow, sc.schedule = 1000.0, 1, _lib.FG_SCHEDULE_RF
        tl = (ctypes.c_double * 3)(0.9, 0.5, 0.0)
        assert L.fg_wan_sampler_run(h, ctypes.byref(sc), fake, tl, 2, _lib.FG_SAMPLE_ODE, None, None, 0, 1, 1, 16, 16, fake, 1 << 40, 0,
                                    None) == FG_EINVAL and word in L.fg_last_error()
        gc = _lib.fg_wan_guided_sampler_config()
        gc.t_scale = 1000.0
        tab8 = (ctypes.c_double * 16)(*([0.5] * 16))
        assert L.fg_wan_guided_sampler_run(h, ctypes.byref(gc), fake, tl, tab8, 2, None, 0, 1, 1, 16, 16, fake, 1 << 40, 0,
                                           None) == FG_EINVAL and word in L.fg_last_error()

        # ---- before packing; the image length's range
        assert L.fg_wan_set_i2v_cond(h, fake, fake, 1, 1, 16, 16, 257, fake, 1 << 30, None) == FG_ENOTREADY and b"not packed" in L.fg_last_error()
        assert L.fg_wan_forward_full(h, fake, fake, None, out, 1, 1, 16, 16, None, 0, fake, 1 << 30, None) == FG_ENOTREADY
        assert L.fg_wan_set_i2v_cond(h, fake, fake, 1, 1, 16, 16, 1025, fake, 1 << 30, None) == FG_EINVAL and b"image_len" in L.fg_last_error()
        assert L.fg_wan_set_i2v_cond(plain, fake, fake, 1, 1, 16, 16, 257, fake, 1 << 30, None) == FG_EINVAL
        assert L.fg_wan_i2v_cond_workspace_bytes(h, 2, 257) > L.fg_wan_i2v_cond_workspace_bytes(h, 2, 1) > 0
        assert L.fg_wan_i2v_cond_workspace_bytes(h, 2, 1025) == 0 and L.fg_wan_i2v_cond_workspace_bytes(plain, 2, 257) == 0
        assert L.fg_wan_i2v_cond_read(h, 0, None, None, None, None) == FG_ENOTREADY and L.fg_wan_i2v_cond_read(h, 2, None, None, None, None) == FG_EINVAL
        # the video of an image-to-video handle has latent_channels channels: the loops' workspaces are the 16-channel network's
        plain16 = ctypes.c_void_p()
        assert L.fg_wan_create_ex(ctypes.byref(_cfg(in_channels=16)), None, ctypes.byref(plain16)) == 0
        made.append(plain16)
        assert L.fg_wan_full_sampler_workspace_bytes(h, 2, 5, 16, 24) == L.fg_wan_full_sampler_workspace_bytes(plain16, 2, 5, 16, 24)
        assert L.fg_wan_full_sampler_workspace_bytes(h, 2, 5, 16, 24) < L.fg_wan_full_sampler_workspace_bytes(plain, 2, 5, 16, 24)
        # the handle-free op's argument checks
        dual = L.fg_op_wan_dual_cross_attention
        assert dual(fake, 256, 0, fake, fake, 512, 0, 37, fake, fake, 512, 0, 257, out, 256, 0, 1, 2, 0, None) == FG_EINVAL
        assert dual(fake, 256, 0, fake, fake, 512, 0, 37, None, fake, 512, 0, 257, out, 256, 0, 1, 2, 8, None) == FG_EINVAL
        assert dual(fake, 252, 0, fake, fake, 512, 0, 37, fake, fake, 512, 0, 257, out, 256, 0, 1, 2, 8, None) == FG_EINVAL
    finally:
        for hh in made:
            L.fg_wan_destroy(hh)


@pytest.mark.parametrize("frames", [1, 2, 5])
def test_mask_reshuffle_is_ones_on_frame_zero(frames):
    assert torch.equal(I.mask_literal(2, frames, 4, 6), I.mask_first_frame(2, frames, 4, 6))
    assert I.mask_literal(2, frames, 4, 6).shape == (2, 4, frames, 4, 6)


@functools.lru_cache(maxsize=None)
def _oracle():
    sd, x, t, cond = I.case()
    return sd, x, t, cond, I.WanI2VRef(sd, I.TINY).forward(x, t, cond)


@pytest.mark.parametrize("mutant", I.MUTANTS)
def test_mutants_stand_apart_on_the_gpu_tests_inputs(mutant):
    """A condition on the inputs of tests/test_gpu_wan_i2v.py::test_forward_against_oracle_and_its_mutants: the oracle and each mutant
    differ by at least MUTANT_FACTOR x TOL in relative L2, so a HIP path within TOL of the oracle is not within reach of a mutant."""
    sd, x, t, cond, want = _oracle()
    d = _rel(I.WanI2VRef(sd, I.TINY, mutant=mutant).forward(x, t, cond), want)
    print("mutant", mutant, d)
    assert d >= MUTANT_FACTOR * TOL, (mutant, d)


def test_reference_without_an_image_is_wan_on_the_concatenated_input():
    import wan_full_ref as W

    sd, x, t, cond = I.case(image_dim=0)
    assert list(sd) == list(R.state_dict_shapes(I.TINY))
    want = W.WanFullRef(sd, I.TINY).forward(torch.cat([x, I.mask_first_frame(*x.shape[:1], *x.shape[2:]), cond["ff"]], dim=1), t, cond["text"])
    assert torch.equal(I.WanI2VRef(sd, I.TINY).forward(x, t, cond), want)


# ---- the module's surface -------------------------------------------------------------------------------------------------------
def _net(**kw):
    from fastgen_amd.networks.WanI2V.network import WanI2V

    return WanI2V(**dict(dict(KW, image_dim=128), **kw))


def test_module_surface():
    from fastgen_amd.networks.WanI2V.network import WanI2V

    net = _net()
    assert list(net.state_dict().keys()) == list(I.state_dict_shapes(I.TINY, 128))
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == I.state_dict_shapes(I.TINY, 128)
    net.load_state_dict(I.random_state_dict(I.TINY, 128, 3), strict=True)
    assert list(_net(image_dim=0).state_dict().keys()) == list(R.state_dict_shapes(I.TINY))
    assert net.is_i2v and net.preserve_conditioning_is_identity and net.concat_mask
    x = torch.zeros(1, 16, 1, 4, 4)
    assert net.preserve_conditioning(x, {"first_frame_cond": x}) is x
    t = torch.tensor([0.5])
    with torch.no_grad():
        with pytest.raises(AssertionError, match="must be a dict"):
            net(x, t, condition=torch.zeros(1, 3, 128))
        with pytest.raises(AssertionError, match="text_embeds"):
            net(x, t, condition={"first_frame_cond": x})
        with pytest.raises(AssertionError, match="first_frame_cond"):
            net(x, t, condition={"text_embeds": torch.zeros(1, 3, 128)})
        with pytest.raises(RuntimeError, match="HIP GPU only"):
            net(x, t, condition={"text_embeds": torch.zeros(1, 3, 128), "first_frame_cond": x})
        with pytest.raises(ValueError, match=r"\[B, 16, F, H, W\]"):
            net._check_video(torch.zeros(1, 36, 1, 4, 4), "x_t")
    for kw in (dict(concat_mask=False), dict(expand_timesteps=True)):
        with pytest.raises(NotImplementedError, match="Wan2.2 TI2V"):
            WanI2V(**dict(KW, **kw))
    with pytest.raises(NotImplementedError, match="pos_embed"):
        WanI2V(**dict(KW, pos_embed_seq_len=514))
    # the plain network keeps its refusal
    from fastgen_amd.networks.Wan.network import Wan

    with pytest.raises(NotImplementedError, match="image conditioning"):
        Wan._text({"text_embeds": None})


def test_generator_fn_takes_the_fused_loop(monkeypatch):
    """A network whose `preserve_conditioning` is the identity stays eligible for the fused loop (methods/model.py)."""
    from fastgen_amd.methods.model import FastGenModel

    net = _net()
    seen = {}

    def few_step_sample(noise, condition, t_list, **kw):
        seen.update(condition=condition, steps=len(t_list) - 1, **kw)
        return noise.clone()

    monkeypatch.setattr(net, "few_step_sample", few_step_sample)
    cond = {"text_embeds": torch.zeros(1, 3, 128), "first_frame_cond": torch.zeros(1, 16, 1, 4, 4)}
    out = FastGenModel.generator_fn(net, torch.ones(1, 16, 1, 4, 4), student_sample_steps=2, condition=cond)  # (the generic loop would need a GPU)
    assert seen["condition"] is cond and seen["steps"] == 2 and seen["loop"] == "x0" and torch.equal(out, torch.ones(1, 16, 1, 4, 4))
