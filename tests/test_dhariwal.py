"""CPU tests of EDMPrecond(model_type="DhariwalUNet"): the module reproduces the reference's in64 state dict, the functional
restatement (tests/dhariwal_ref.py) reproduces the fixture recorded from the reference, the unsupported paths refuse loudly, and a
zero-initialised fg_edm_config still means SongUNet."""
import ctypes
import os

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks.EDM.network import EDMPrecond
from oracle import edm_ref as R

import dhariwal_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SONG_KW = dict(img_resolution=32, img_channels=3, label_dim=10, sigma_shift=0.0, sigma_data=0.5, model_type="SongUNet",
               augment_dim=9, model_channels=128, channel_mult=[2, 2, 2], channel_mult_noise=1, embedding_type="positional",
               encoder_type="standard", decoder_type="standard", resample_filter=[1, 1], dropout=0.0, label_dropout=0,
               r_timestep=False, drop_precond=None)


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def recorded_keys():
    out = []
    for line in open(os.path.join(GOLDEN, "dhariwal_in64_state_dict_keys.txt")):
        name, shape = line.split()
        out.append((name, tuple(int(s) for s in shape.split(","))))
    return out


def test_in64_state_dict_matches_reference():
    net = EDMPrecond(**D.IN64.kwargs())
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    want = recorded_keys()
    assert len(want) == 555
    assert got == want
    assert sum(p.numel() for p in net.parameters()) == sum(
        torch.Size(s).numel() for k, s in want if not k.endswith("resample_filter"))


def test_reference_defaults():
    """DhariwalUNet's own constructor defaults (EDM/network.py:585-600) apply when the kwargs leave them out."""
    kw = {k: v for k, v in D.IN64.kwargs().items()
          if k not in ("model_channels", "channel_mult", "channel_mult_emb", "num_blocks", "attn_resolutions", "dropout")}
    net = EDMPrecond(**kw)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == recorded_keys()
    assert net.dropout == 0.10


def test_in64_state_dict_loads_strict():
    net = EDMPrecond(**D.IN64.kwargs())
    sd = {k: torch.zeros(s) for k, s in recorded_keys()}
    net.load_state_dict(sd, strict=True)


def test_state_shapes_restatement():
    assert [(k, tuple(s)) for k, s in D.state_shapes(D.IN64).items()] == recorded_keys()


@pytest.fixture(scope="module")
def narrow():
    fx = torch.load(os.path.join(GOLDEN, "dhariwal_narrow_b2.pt"))
    sd = D.random_state_dict(D.NARROW, seed=1234)
    return fx, sd


def test_restatement_forward_matches_reference(narrow):
    fx, sd = narrow
    cfg = D.NARROW
    x = seeded((2, 3, 64, 64), 11) * fx["t"].reshape(-1, 1, 1, 1).float()
    assert torch.equal(D.subsample(x), fx["x_check"])
    trace = {}
    with torch.no_grad():
        out = D.precond_forward(sd, cfg, x, fx["t"], fx["cond"], trace=trace)
        out_nl = D.precond_forward(sd, cfg, x, fx["t"], None)
    assert (out - fx["out"]).abs().max().item() <= 1e-6
    assert (D.subsample(out_nl) - fx["out_nolabel"]).abs().max().item() <= 1e-6
    assert (trace["emb"] - fx["emb"]).abs().max().item() <= 1e-6
    assert set(fx["blocks"]) == {k for k in trace if k != "emb"}
    for k, v in fx["blocks"].items():
        ref = v.abs().max().item()
        assert (D.subsample(trace[k]) - v).abs().max().item() <= 1e-6 * max(1.0, ref), k


def test_restatement_generator_matches_reference(narrow):
    fx, sd = narrow
    noise = seeded((2, 3, 64, 64), 21)
    eps = [seeded((2, 3, 64, 64), s) for s in (22, 23, 24)]
    for steps in (1, 4):
        got = D.generator_fn(sd, D.NARROW, noise, fx["cond"], steps, "sde", eps_list=eps)
        assert (got - fx["gen"][f"sde{steps}"]).abs().max().item() <= 1e-6, steps
    got = D.generator_fn(sd, D.NARROW, noise, fx["cond"], 2, "ode")
    assert (got - fx["gen"]["ode2"]).abs().max().item() <= 1e-6
    got = D.generator_fn(sd, D.NARROW, noise, fx["cond"], 2, "ode", t_list=[80.0, 1.5, 0.0])
    assert (D.subsample(got) - fx["gen"]["tlist2"]).abs().max().item() <= 1e-6


@pytest.mark.parametrize("key,value", [("embedding_type", "positional"), ("channel_mult_noise", 1), ("encoder_type", "standard"),
                                       ("decoder_type", "standard"), ("resample_filter", [1, 1])])
def test_songunet_keywords_refused(key, value):
    with pytest.raises(ValueError):
        EDMPrecond(**{**D.NARROW.kwargs(), key: value})


def test_unsupported_paths_refuse():
    with pytest.raises(NotImplementedError):
        EDMPrecond(**D.NARROW.kwargs(), compute_dtype="fp32")
    with pytest.raises(NotImplementedError):
        EDMPrecond(**{**D.NARROW.kwargs(), "r_timestep": True})
    net = EDMPrecond(**D.NARROW.kwargs())
    x, t = torch.zeros(1, 3, 64, 64), torch.ones(1)
    with pytest.raises(NotImplementedError):
        net(x, t, feature_indices={0})
    with pytest.raises(NotImplementedError):
        net(x, t, return_features_early=True, feature_indices={0})
    with pytest.raises(NotImplementedError):  # autograd through the network
        net(x, t)
    with pytest.raises(NotImplementedError):
        net.fully_shard()
    with pytest.raises(NotImplementedError):
        net.jvp(x, t, x)
    net.requires_grad_(False)
    with pytest.raises(NotImplementedError):  # train() mode with dropout draws a mask: a training forward
        EDMPrecond(**{**D.NARROW.kwargs(), "dropout": 0.1}).requires_grad_(False).train()(x, t)
    net.compute_dtype = "fp32"
    with pytest.raises(NotImplementedError):
        net(x, t)


def _create(cfg):
    h = ctypes.c_void_p()
    rc = _lib.lib().fg_edm_create(ctypes.byref(cfg), ctypes.byref(h))
    return rc, h


def _song_cfg():
    c = _lib.fg_edm_config()  # zero-initialised: model_type 0
    c.img_resolution, c.img_channels, c.label_dim, c.augment_dim, c.model_channels = 32, 3, 10, 9, 128
    c.num_levels, c.channel_mult_emb, c.num_blocks, c.num_attn_resolutions, c.channel_mult_noise = 3, 4, 4, 1, 1
    for i in range(3):
        c.channel_mult[i] = 2
    c.attn_resolutions[0] = 16
    c.sigma_data = 0.5
    c.compute_dtype = _lib.FG_DTYPE_BF16X3
    return c


def test_zero_config_is_songunet():
    L = _lib.lib()
    c = _song_cfg()
    assert c.model_type == _lib.FG_MODEL_SONGUNET == 0
    rc, h = _create(c)
    assert rc == 0
    try:
        names = []
        name = ctypes.c_char_p()
        for i in range(L.fg_edm_num_params(h)):
            _lib.check(L.fg_edm_param_info(h, i, ctypes.byref(name), None, None))
            names.append(name.value.decode())
        want = [k for k in R.param_shapes(R.CIFAR10) if not k.endswith("resample_filter")]
        assert names == want
    finally:
        L.fg_edm_destroy(h)


def _narrow_cfg():
    cfg = D.NARROW
    c = _lib.fg_edm_config()
    c.img_resolution, c.img_channels, c.label_dim, c.augment_dim, c.model_channels = 64, 3, cfg.label_dim, cfg.augment_dim, 64
    c.num_levels, c.channel_mult_emb, c.num_blocks, c.num_attn_resolutions, c.channel_mult_noise = 4, 4, 1, 3, 1
    for i, m in enumerate(cfg.channel_mult):
        c.channel_mult[i] = m
    for i, r in enumerate(cfg.attn_resolutions):
        c.attn_resolutions[i] = r
    c.sigma_data, c.compute_dtype, c.model_type = 0.5, _lib.FG_DTYPE_BF16X3, _lib.FG_MODEL_DHARIWAL
    return c


def test_dhariwal_handle_param_order_and_refusals():
    L = _lib.lib()
    cfg = D.NARROW
    c = _narrow_cfg()
    rc, h = _create(c)
    assert rc == 0, _lib.lib().fg_last_error()
    try:
        name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 4)()
        got = []
        for i in range(L.fg_edm_num_params(h)):
            _lib.check(L.fg_edm_param_info(h, i, ctypes.byref(name), ctypes.byref(ndim), shape))
            got.append((name.value.decode(), tuple(shape[j] for j in range(ndim.value))))
        want = [(k, tuple(s)) for k, s in D.state_shapes(cfg).items() if not k.endswith("resample_filter")]
        assert got == want
        assert L.fg_edm_num_feature_taps(h) == 0
        assert L.fg_edm_backward_workspace_bytes(h, 2) == 0
        assert L.fg_edm_workspace_bytes(h, 2) > 0
    finally:
        L.fg_edm_destroy(h)
    for bad in (dict(compute_dtype=_lib.FG_DTYPE_F32), dict(r_timestep=1), dict(model_type=2), dict(img_resolution=128)):
        c2 = _lib.fg_edm_config.from_buffer_copy(c)
        for k, v in bad.items():
            setattr(c2, k, v)
        rc, h = _create(c2)
        assert rc != 0, bad


def test_dhariwal_block_list_and_run_block_refusals():
    """fg_edm_num_blocks / fg_edm_block_info on an ADM handle list D.layout's encoder then decoder blocks; fg_edm_run_block refuses a
    c1 / c2 split other than (cin - skip, skip) before it looks at the (here unpacked, device-less) weights."""
    L = _lib.lib()
    _, enc, dec = D.layout(D.NARROW)
    rc, h = _create(_narrow_cfg())
    assert rc == 0, L.fg_last_error()
    try:
        assert L.fg_edm_num_blocks(h) == len(enc) + len(dec) == 20
        kp, ci, co, ri, ro, at = (ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int())
        blocks = [("enc", b) for b in enc] + [("dec", b) for b in dec]
        prev_cout = None
        dummy = ctypes.create_string_buffer(64)  # a non-null pointer: the refusals come before any use of it
        for i, (side, b) in enumerate(blocks):
            _lib.check(L.fg_edm_block_info(h, i, ctypes.byref(kp), ctypes.byref(ci), ctypes.byref(co), ctypes.byref(ri), ctypes.byref(ro),
                                           ctypes.byref(at)))
            assert kp.value.decode() == f"model.{side}.{b.key}"
            assert (ci.value, co.value, ro.value, bool(at.value)) == (b.cin, b.cout, b.res, b.attn), b.key
            assert ri.value == (2 * b.res if b.down else b.res // 2 if b.up else b.res), b.key
            skip = b.cin - prev_cout if side == "dec" and b.cin != prev_cout else 0
            prev_cout = b.cout
            p = ctypes.cast(dummy, ctypes.c_void_p)
            for c1, c2 in ((b.cin - skip + 32, skip - 32) if skip else (b.cin - 32, 32), (b.cin + 64, 0), (0, b.cin), (b.cin, skip or 64)):
                assert L.fg_edm_run_block(h, i, p, c1, p, c2, p, p, 2, p, 64, None) == 1, (b.key, c1, c2)
                assert b"channel split" in L.fg_last_error(), L.fg_last_error()
            # the right split gets past the argument checks: the weights are not packed
            assert L.fg_edm_run_block(h, i, p, b.cin - skip, p, skip, p, p, 2, p, 64, None) == 2, L.fg_last_error()
        assert L.fg_edm_block_info(h, len(blocks), None, None, None, None, None, None) == 1
        assert L.fg_edm_block_info(h, -1, None, None, None, None, None, None) == 1
    finally:
        L.fg_edm_destroy(h)


def test_adm_op_refusals():
    """The fg_op_adm_* entry points refuse unsupported shapes, modes and pointers with FG_EINVAL before launching anything (this
    runs without a GPU); the byte counts follow the documented layouts."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 64)  # 64-byte aligned, never dereferenced here
    odd = ctypes.c_void_p(p.value + 4)
    assert L.fg_op_adm_conv_pack_bytes(2, 200, 96, 3) == 256 * 9 * 96 * 2 * 2
    assert L.fg_op_adm_conv_pack_bytes(1, 3, 32, 1) == 64 * 32 * 2
    for bad in ((0, 64, 64, 3), (1, 64, 64, 2), (2, 0, 64, 1), (2, 64, 48, 1)):
        assert L.fg_op_adm_conv_pack_bytes(*bad) == 0, bad
        assert L.fg_op_adm_conv_pack(bad[0], p, p, bad[1], bad[2], bad[3], None) == 1, bad
    assert L.fg_op_adm_conv_pack(2, None, p, 64, 64, 3, None) == 1

    def conv(**kw):
        a = dict(mode=2, ks=3, src1=p, c1=64, src2=None, c2=0, batch=1, hs=8, h=8, res_mode=0, ab=None, silu=0, packed=p, bias=None,
                 resid=None, resid_mode=0, out=p, cout=64)
        a.update(kw)
        return L.fg_op_adm_conv(*a.values(), None)

    for kw in (dict(mode=0), dict(ks=5), dict(c1=48), dict(c1=0, src2=p, c2=64), dict(c2=32), dict(c2=16, src2=p), dict(cout=0),
               dict(batch=0), dict(res_mode=1), dict(res_mode=2), dict(res_mode=3, hs=8), dict(res_mode=1, hs=8, h=4, src1=None),
               dict(resid=p, resid_mode=3), dict(resid=p, resid_mode=2, hs=9, h=9), dict(src1=odd), dict(packed=None), dict(out=None)):
        assert conv(**kw) == 1, kw
    assert L.fg_op_adm_gn_workspace_bytes(3, 200, 192) == 3 * 3 * 96 * 8  # slots of 64+ pixels, one float2 per channel pair
    assert L.fg_op_adm_gn_workspace_bytes(2, 127, 64) == 2 * 1 * 32 * 8

    def gn(c1, c2, hw=64, temb=None, stride=0, ws=1 << 12, x1=p):
        return L.fg_op_adm_gn_coeffs(x1, c1, p if c2 else None, c2, p, p, 1e-5, temb, stride, p, 1, hw, p, ws, None)

    assert gn(63, 1) == 1 and b"even" in L.fg_last_error()      # c1 odd
    assert gn(160, 0) == 1 and b"group size" in L.fg_last_error()  # 32 groups of 5
    assert gn(130, 0) == 1 and b"group size" in L.fg_last_error()  # 130 % 32 != 0
    assert gn(4, 2) == 1                                           # fewer than 8 channels
    assert gn(64, 0, hw=0) == 1
    assert gn(64, 0, temb=p, stride=127) == 1                     # temb_stride < 2 C
    assert gn(64, 0, hw=4096, ws=63 * 32 * 8) == 1                 # workspace one slot short
    assert gn(64, 0, x1=odd) == 1
    for t, heads, batch in ((96, 1, 1), (0, 1, 1), (64, 0, 1), (64, 1, 0)):
        assert L.fg_op_adm_attention(p, p, batch, t, heads, None) == 1, (t, heads, batch)
    assert L.fg_op_adm_attention(None, p, 1, 64, 1, None) == 1
    for n, aug, wa, ad in ((63, None, None, 0), (0, None, None, 0), (64, p, None, 9), (64, p, p, 0)):
        assert L.fg_op_adm_map_in(p, p, aug, wa, ad, p, 2, n, None) == 1, (n, ad)
