"""CPU side of the video-to-video network (fg_wan_create_vace, fastgen_amd.networks.VaceWan): the parameter table against
tests/wan_vace_ref.py, the refusals the C ABI makes from its arguments alone, the consumption order of the hints against a literal
transcription of the reference's pop loop, the distance of the oracle's mutants on the inputs the GPU forward test uses, and the
module's surface.  Nothing here touches a GPU."""
import ctypes
import functools

import pytest
import torch

from oracle import wan_ref as R
import wan_full_ref as W
import wan_vace_ref as V

FG_EINVAL, FG_ENOTREADY = 1, 2
TOL, MUTANT_FACTOR = 2e-2, 5.0  # tests/test_gpu_wan_vace.py's forward tolerance; the project's factor (tests/test_gpu_wan_blocks.py)
KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=3, vace_layers=(0, 2))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _cfg(num_layers=3):
    from fastgen_amd import _lib

    c = _lib.fg_wan_config()
    c.num_heads, c.head_dim, c.in_channels, c.out_channels, c.text_dim, c.freq_dim = 2, 128, 16, 16, 128, 256
    c.ffn_dim, c.num_layers, c.rope_max_seq_len, c.chunk_size, c.total_num_frames, c.eps = 512, num_layers, 1024, 1, 1, 1e-6
    return c


def _vace(layers=(0, 2), channels=96, n=None):
    from fastgen_amd import _lib

    v = _lib.fg_wan_vace_config()
    v.vace_in_channels, v.num_vace_layers = channels, len(layers) if n is None else n
    for j, i in enumerate(layers):
        v.vace_layers[j] = i
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
    assert ctypes.sizeof(_lib.fg_wan_vace_config) == 66 * 4
    made = []

    def create(cfg, vace, ext=None):
        h = ctypes.c_void_p()
        rc = L.fg_wan_create_vace(ctypes.byref(cfg), ctypes.byref(ext) if ext is not None else None, ctypes.byref(vace), ctypes.byref(h))
        if rc == 0:
            made.append(h)
        return rc, h

    try:
        # ---- the table: the oracle's keys and shapes in order; the plain network's table with insertions at the two named places
        rc, h = create(_cfg(), _vace())
        assert rc == 0
        tab = _table(L, h)
        want = V.state_dict_shapes(V.TINY)
        assert [n for n, _ in tab] == list(want) and dict(tab) == want
        plain = ctypes.c_void_p()
        assert L.fg_wan_create_ex(ctypes.byref(_cfg()), None, ctypes.byref(plain)) == 0
        made.append(plain)
        base = _table(L, plain)
        per_block = sum(1 for n, _ in base if n.startswith("transformer.blocks.0."))
        assert [e for e in tab if e in base] == base and len(tab) == len(base) + 2 + 2 * (per_block + 2) + 2
        names = [n for n, _ in tab]
        at = names.index("transformer.patch_embedding.bias")
        assert names[at + 1: at + 3] == ["transformer.vace_patch_embedding.weight", "transformer.vace_patch_embedding.bias"]
        at = names.index("transformer.blocks.2.ffn.net.2.bias")
        assert names[at + 1: at + 4] == ["transformer.vace_blocks.0.scale_shift_table", "transformer.vace_blocks.0.proj_in.weight",
                                         "transformer.vace_blocks.0.proj_in.bias"]
        assert names[names.index("transformer.proj_out.weight") - 1] == "transformer.vace_blocks.1.proj_out.bias"
        assert "transformer.vace_blocks.1.proj_in.weight" not in names
        ext = _lib.fg_wan_ext_config()
        ext.r_timestep, ext.time_cond_diff = 1, 0
        rc, hr = create(_cfg(), _vace(), ext)
        assert rc == 0 and [n for n, _ in _table(L, hr)] == list(V.state_dict_shapes(V.TINY, r_timestep=True))

        # ---- creation refusals, each naming its field
        for cfg, vace, word in ((_cfg(), _vace((2, 0)), b"vace_layers"), (_cfg(), _vace((0, 0)), b"vace_layers"), (_cfg(), _vace((0, 3)), b"vace_layers"),
                                (_cfg(), _vace((-1, 2)), b"vace_layers"), (_cfg(), _vace((), n=0), b"num_vace_layers"),
                                (_cfg(), _vace((0,), n=65), b"num_vace_layers"), (_cfg(), _vace(channels=0), b"vace_in_channels"),
                                (_cfg(), _vace(channels=129), b"vace_in_channels")):
            rc, hb = create(cfg, vace)
            assert rc == FG_EINVAL and not hb.value and word in L.fg_last_error(), word
        hb = ctypes.c_void_p()
        assert L.fg_wan_create_vace(ctypes.byref(_cfg()), None, None, ctypes.byref(hb)) == FG_EINVAL

        # ---- the chunked / causal entry points on a VACE handle
        fake, out = ctypes.c_void_p(4096), ctypes.c_void_p(8192)  # non-null, 256-byte aligned, never dereferenced
        word = b"not implemented for a VACE handle"
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

        # ---- the taps: num_layers + k on a VACE handle only
        taps = (_lib.fg_wan_block_taps * 1)()
        idx = (ctypes.c_int * 1)(3)
        assert L.fg_wan_forward_full_features(plain, fake, fake, None, out, 1, 1, 16, 16, None, 0, idx, taps, 1, None, None, None, fake, 1 << 30,
                                              None) == FG_EINVAL and b"tap_blocks" in L.fg_last_error()
        idx[0] = 5
        assert L.fg_wan_forward_full_features(h, fake, fake, None, out, 1, 1, 16, 16, None, 0, idx, taps, 1, None, None, None, fake, 1 << 30,
                                              None) == FG_EINVAL and b"tap_blocks" in L.fg_last_error()
        idx[0] = 4  # (a valid index: the call gets as far as the packing check)
        assert L.fg_wan_forward_full_features(h, fake, fake, None, out, 1, 1, 16, 16, None, 0, idx, taps, 1, None, None, None, fake, 1 << 30,
                                              None) == FG_ENOTREADY

        # ---- the setters: before packing, on another handle, bad arguments
        assert L.fg_wan_set_vace_context(h, fake, 1, 2, 2, 16, 16, fake, 1 << 30, None) == FG_ENOTREADY and b"not packed" in L.fg_last_error()
        assert L.fg_wan_set_vace_context(h, fake, 1, 2, 3, 16, 16, fake, 1 << 30, None) == FG_EINVAL and b"ctx_frames" in L.fg_last_error()
        assert L.fg_wan_set_vace_context(h, fake, 1, 2, 2, 15, 16, fake, 1 << 30, None) == FG_EINVAL
        assert L.fg_wan_set_vace_context(plain, fake, 1, 2, 2, 16, 16, fake, 1 << 30, None) == FG_EINVAL
        assert L.fg_wan_vace_context_read(h, fake, None) == FG_ENOTREADY and L.fg_wan_vace_context_read(plain, fake, None) == FG_EINVAL
        assert L.fg_wan_vace_context_workspace_bytes(h, 2, 5, 16, 24) == 2 * 480 * 256 * 2 and L.fg_wan_vace_context_workspace_bytes(plain, 2, 5, 16, 24) == 0
        two, three = (ctypes.c_float * 2)(0.5, 1.5), (ctypes.c_float * 3)(1, 1, 1)
        assert L.fg_wan_set_vace_scale(h, two, 2, None) == 0  # (before the first pack: kept on the host)
        assert L.fg_wan_set_vace_scale(h, three, 3, None) == FG_EINVAL and L.fg_wan_set_vace_scale(plain, two, 2, None) == FG_EINVAL
        assert L.fg_wan_forward_full(h, fake, fake, None, out, 1, 1, 16, 16, None, 0, fake, 1 << 30, None) == FG_ENOTREADY
        # the workspace grows by the control stream's ping-pong pair on a VACE handle only, whatever the number of VACE layers
        grow = L.fg_wan_full_workspace_bytes(h, 2, 5, 16, 24) - L.fg_wan_full_workspace_bytes(plain, 2, 5, 16, 24)
        assert grow == 2 * (2 * 480 * 256 * 2)
        rc, h3 = create(_cfg(), _vace((0, 1, 2)))
        assert rc == 0 and L.fg_wan_full_workspace_bytes(h3, 2, 5, 16, 24) == L.fg_wan_full_workspace_bytes(h, 2, 5, 16, 24)
        assert L.fg_wan_full_sampler_workspace_bytes(h, 2, 5, 16, 24) - L.fg_wan_full_sampler_workspace_bytes(plain, 2, 5, 16, 24) == grow
        assert L.fg_wan_workspace_bytes(h, 2, 5, 16, 24) == L.fg_wan_workspace_bytes(plain, 2, 5, 16, 24)
        # the handle-free op's argument checks
        op = L.fg_op_wan_vace_patch_embed
        assert op(fake, fake, fake, out, 1, 129, 1, 16, 16, 256, 0, None) == FG_EINVAL
        assert op(fake, fake, fake, out, 1, 48, 1, 16, 16, 256, 2, None) == FG_EINVAL and b"96 channels" in L.fg_last_error()
        assert op(fake, fake, fake, out, 1, 96, 1, 15, 16, 256, 0, None) == FG_EINVAL
        assert L.fg_op_wan_patch_embed(fake, None, fake, fake, out, 1, 96, 1, 16, 16, 256, 0, None) == FG_EINVAL  # (keeps its 64-channel bound)
    finally:
        for hh in made:
            L.fg_wan_destroy(hh)


@pytest.mark.parametrize("num_layers,vace_layers,skip", [(3, (0, 2), None), (3, (0, 2), [0]), (3, (0, 2), [2]), (3, (0, 2), [0, 2]), (3, (0, 2), [1]),
                                                         (6, (0, 2, 4), [2]), (6, (1, 3, 5), [0, 1]), (4, (0, 1, 2, 3), [1, 2])])
def test_consumption_order_is_the_pop_loops(num_layers, vace_layers, skip):
    """The j-th EXECUTED VACE layer receives hint j: the oracle's main loop against the literal pop loop, on indices."""
    got = V.consumption_literal(num_layers, vace_layers, skip)
    executed = [i for i in vace_layers if not (skip and i in skip)]
    assert got == [(i, j) for j, i in enumerate(executed)]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    sd, x, t, cond, skip = V.case(name)
    return sd, x, t, cond, skip, V.WanVaceRef(sd, V.TINY, torch.float64, context_scale=V.SCALES).forward(x, t, cond, skip_layers=skip)


@pytest.mark.parametrize("mutant", V.MUTANTS)
def test_mutants_stand_apart_on_the_gpu_tests_inputs(mutant):
    """A condition on the inputs of tests/test_gpu_wan_vace.py::test_forward_against_oracle_and_its_mutants: the fp64 oracle and each
    mutant differ by at least MUTANT_FACTOR x TOL in relative L2 on the case that exposes the mutant, so a HIP path within TOL of the
    oracle is not within reach of it."""
    sd, x, t, cond, skip, want = _oracle(V.EXPOSED_BY[mutant])
    d = _rel(V.WanVaceRef(sd, V.TINY, torch.float64, context_scale=V.SCALES, mutant=mutant).forward(x, t, cond, skip_layers=skip), want)
    print("mutant", mutant, V.EXPOSED_BY[mutant], d)
    assert d >= MUTANT_FACTOR * TOL, (mutant, d)


def test_mutants_that_need_their_case_are_silent_elsewhere():
    """hint_by_layer_index differs only under skip_layers, pad_after_proj_in only with a context shorter than the video."""
    sd, x, t, cond, skip, want = _oracle("full")
    for mutant in ("hint_by_layer_index", "pad_after_proj_in"):
        assert torch.equal(V.WanVaceRef(sd, V.TINY, torch.float64, context_scale=V.SCALES, mutant=mutant).forward(x, t, cond), want)


def test_oracle_with_zero_scales_is_wan():
    sd, x, t, cond, _ = V.case("full")
    plain = {k: v for k, v in sd.items() if k in W.state_dict_shapes(V.TINY)}
    want = W.WanFullRef(plain, V.TINY).forward(x, t, cond["text"])
    assert torch.equal(V.WanVaceRef(sd, V.TINY, context_scale=0.0).forward(x, t, cond), want)
    assert list(plain) == list(R.state_dict_shapes(V.TINY))


def test_padded_rows_of_ctx_in_are_the_bias():
    sd, x, t, cond, _ = V.case("short")
    ref = V.WanVaceRef(sd, V.TINY, torch.float64)
    c = ref.ctx_in(cond["ctx"], 480)
    assert c.shape == (2, 480, 256) and torch.equal(c[:, 3 * 96:], ref.p["vace_blocks.0.proj_in.bias"].expand(2, 480 - 3 * 96, 256))


# ---- the module's surface -------------------------------------------------------------------------------------------------------
def _net(**kw):
    from fastgen_amd.networks.VaceWan.network import VACEWan

    return VACEWan(**dict(KW, **kw))


def test_module_surface():
    from fastgen_amd.networks.VaceWan.network import CausalVACEWan, VACEWan

    net = _net(context_scale=[0.5, 1.5], depth_model_path="somewhere")
    assert list(net.state_dict().keys()) == list(V.state_dict_shapes(V.TINY))
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == V.state_dict_shapes(V.TINY)
    net.load_state_dict(V.random_state_dict(V.TINY, 3), strict=True)
    assert list(_net(r_timestep=True).state_dict().keys()) == list(V.state_dict_shapes(V.TINY, r_timestep=True))
    assert net.is_vid2vid and net.time_cond_type == "abs" and net.depth_model_path == "somewhere" and net.vace_layers == (0, 2)
    assert not hasattr(net, "preserve_conditioning")
    assert VACEWan(**dict(KW, vace_layers=None, num_layers=4)).vace_layers == (0, 2)
    x = torch.zeros(1, 16, 2, 4, 4)
    ctx = torch.zeros(1, 96, 2, 4, 4)
    text = torch.zeros(1, 3, 128)
    t = torch.tensor([0.5])
    with torch.no_grad():
        with pytest.raises(AssertionError, match="must be a dict"):
            net(x, t, condition=text)
        with pytest.raises(AssertionError, match="text_embeds"):
            net(x, t, condition={"vid_context": ctx})
        with pytest.raises(AssertionError, match="vid_context"):
            net(x, t, condition={"text_embeds": text})
        with pytest.raises(RuntimeError, match="HIP GPU only"):
            net(x, t, condition={"text_embeds": text, "vid_context": ctx})
        net.context_scale = [1.0, 2.0, 3.0]
        with pytest.raises(ValueError, match=r"Length of `control_hidden_states_scale` 3 does not match number of layers 2\."):
            net(x, t, condition={"text_embeds": text, "vid_context": ctx})
        net.context_scale = torch.ones(1)
        with pytest.raises(ValueError, match=r"Length of `control_hidden_states_scale` 1 does not match number of layers 2\."):
            net(x, t, condition={"text_embeds": text, "vid_context": ctx})
        net.context_scale = 2
        assert net._scales() == [2.0, 2.0]
        for bad, word in ((torch.zeros(1, 96, 2, 4, 6), "height and width"), (torch.zeros(1, 96, 3, 4, 4), "more frames"),
                          (torch.zeros(1, 48, 2, 4, 4), r"\[1, 96, Fc, H, W\]")):
            with pytest.raises(ValueError, match=word):
                net._set_context(bad, 1, 2, 4, 4, torch.device("cpu"))
    for kw in (dict(vace_layers=(2, 0)), dict(vace_layers=(0, 3)), dict(vace_layers=()), dict(vace_in_channels=0)):
        with pytest.raises(ValueError):
            VACEWan(**dict(KW, **kw))
    with pytest.raises(NotImplementedError, match="CausalVACEWan"):
        CausalVACEWan()
    # the helpers
    a, b = torch.randn(2, 16, 3, 4, 4), torch.randn(2, 16, 3, 4, 4)
    c = VACEWan.vace_context(a, b)
    assert c.shape == (2, 96, 3, 4, 4) and torch.equal(c[:, :16], a) and torch.equal(c[:, 16:32], b) and bool((c[:, 32:] == 1).all())
    with pytest.raises(NotImplementedError, match="depth annotator"):
        net.prepare_vid_conditioning(torch.zeros(2, 3, 9, 32, 32))
    with pytest.raises(NotImplementedError, match="VAE"):
        net.prepare_vid_conditioning(a, condition_latents=b)
    net._all_zero_latent = a
    assert torch.equal(net.prepare_vid_conditioning(a, condition_latents=b), c)
    # the plain network keeps its refusal of a condition dict
    from fastgen_amd.networks.Wan.network import Wan

    with pytest.raises(NotImplementedError, match="image conditioning"):
        Wan._text({"text_embeds": None})


def test_generator_fn_takes_the_fused_loop(monkeypatch):
    """The network has no `preserve_conditioning` hook: FastGenModel.generator_fn keeps the fused loop and hands it the condition dict."""
    from fastgen_amd.methods.model import FastGenModel

    net = _net()
    seen = {}

    def few_step_sample(noise, condition, t_list, **kw):
        seen.update(condition=condition, steps=len(t_list) - 1, **kw)
        return noise.clone()

    monkeypatch.setattr(net, "few_step_sample", few_step_sample)
    cond = {"text_embeds": torch.zeros(1, 3, 128), "vid_context": torch.zeros(1, 96, 1, 4, 4)}
    out = FastGenModel.generator_fn(net, torch.ones(1, 16, 1, 4, 4), student_sample_steps=2, condition=cond)
    assert seen["condition"] is cond and seen["steps"] == 2 and seen["loop"] == "x0" and torch.equal(out, torch.ones(1, 16, 1, 4, 4))
