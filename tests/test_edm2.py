"""CPU tests of EDM2Precond: state dict against the reference-recorded list, strict load, the functional restatement against the
reference-recorded fixtures, the refusals, and the fg_edm2_* plan / envelope / block entry points (host-only calls)."""
import ctypes
import os

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks.EDM2.network import EDM2Precond

import edm2_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def recorded_keys():
    out = []
    with open(os.path.join(GOLDEN, "edm2_in64_s_state_dict_keys.txt")) as f:
        for line in f:
            k, s = line.split()
            out.append((k, tuple(int(v) for v in s.split(","))))
    return out


def test_state_dict_matches_reference():
    net = EDM2Precond(img_resolution=64, img_channels=3, label_dim=1000)
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    want = recorded_keys()
    assert len(want) == 203 and got == want
    assert [(k, v) for k, v in D.state_shapes(D.IN64_S).items()] == want
    bufs = [k for k, _ in net.named_buffers()]
    assert bufs == ["unet.emb_fourier.freqs", "unet.emb_fourier.phases", "logvar_fourier.freqs", "logvar_fourier.phases"]
    assert abs(sum(v.numel() for v in net.state_dict().values()) / 1e6 - 280.2) < 0.05


def test_strict_load_and_forced_weight_normalization():
    sd = D.random_state_dict(D.NARROW, seed=3)
    net = EDM2Precond(**D.NARROW.kwargs())
    net.load_state_dict(sd, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    v0 = net.unet.enc._modules["64x64_block0"].conv_res0.weight._version
    net.forced_weight_normalization()
    w = net.unet.enc._modules["64x64_block0"].conv_res0.weight
    assert w._version != v0
    assert torch.allclose(w, D.unit_rows(sd["unet.enc.64x64_block0.conv_res0.weight"]), rtol=1e-6, atol=1e-6)
    assert torch.equal(net.unet.out_gain, sd["unet.out_gain"])  # gains are not weights


def test_restatement_against_fixtures():
    fx = torch.load(os.path.join(GOLDEN, "edm2_narrow_b2.pt"))
    sd = D.random_state_dict(D.NARROW, seed=1234)
    assert (sd["unet.out_gain"] != 0).all() and all((v != 0).all() for k, v in sd.items() if k.endswith("emb_gain"))
    x = seeded((2, 3, 64, 64), 11) * fx["t"].reshape(-1, 1, 1, 1).float()
    trace = {}
    with torch.no_grad():
        out = D.precond_forward(sd, D.NARROW, x, fx["t"], fx["cond"], trace=trace)
        assert (out - fx["out"]).abs().max().item() <= 1e-5
        assert (trace["emb"] - fx["emb"]).abs().max().item() <= 1e-6
        assert set(fx["blocks"]) == {b.key for b in sum(D.layout(D.NARROW)[:2], [])}
        for k, v in fx["blocks"].items():
            assert (D.subsample(trace[k]) - v).abs().max().item() <= 1e-5, k
        nl = D.precond_forward(sd, D.NARROW, x, fx["t"], None)
        assert (D.subsample(nl) - fx["out_nolabel"]).abs().max().item() <= 1e-5
        assert (D.logvar(sd, fx["t"]) - fx["logvar"]).abs().max().item() <= 1e-6
    assert fx["out"].abs().max() > 0.1 and fx["gen"]["sde4"].abs().max() > 0.1


def test_refusals():
    kw = D.NARROW.kwargs()
    for bad in (dict(r_timestep=True), dict(embedding_type="positional"), dict(channels_per_head=32), dict(resample_filter=[1, 3, 3, 1]),
                dict(compute_dtype="fp32")):
        with pytest.raises(NotImplementedError):
            EDM2Precond(**{**kw, **bad})
    net = EDM2Precond(**kw)
    x, t = torch.zeros(1, 3, 64, 64), torch.ones(1)
    with pytest.raises(NotImplementedError):
        net(x, t)  # autograd through the network (parameters require grad)
    with pytest.raises(NotImplementedError):
        net.jvp(x, t, x)
    with pytest.raises(NotImplementedError):
        net.fully_shard()
    with torch.no_grad(), pytest.raises(NotImplementedError):
        net(x, t, feature_indices={0})
    with torch.no_grad(), pytest.raises(NotImplementedError):
        net(x, t, return_features_early=True, feature_indices={0})
    drop = EDM2Precond(**kw, dropout=0.1).train()
    with torch.no_grad(), pytest.raises(NotImplementedError):
        drop(x, t)
    fp32 = EDM2Precond(**kw)
    fp32.compute_dtype = "fp32"
    with pytest.raises(NotImplementedError):
        fp32._select_dtype()
    with pytest.raises(ValueError):
        net(x, t, r=t)


def _handle(cfg_py=D.NARROW, **over):
    c = _lib.fg_edm2_config()
    c.img_resolution, c.img_channels, c.label_dim = cfg_py.img_resolution, cfg_py.img_channels, cfg_py.label_dim
    c.model_channels = cfg_py.model_channels
    c.num_levels = len(cfg_py.channel_mult)
    for i, m in enumerate(cfg_py.channel_mult):
        c.channel_mult[i] = m
    c.num_blocks = cfg_py.num_blocks
    c.num_attn_resolutions = len(cfg_py.attn_resolutions)
    for i, a in enumerate(cfg_py.attn_resolutions):
        c.attn_resolutions[i] = a
    c.label_balance = c.concat_balance = 0.5
    c.res_balance = c.attn_balance = 0.3
    c.clip_act, c.sigma_data = 256.0, 0.5
    c.compute_dtype = _lib.FG_DTYPE_BF16X3
    for k, v in over.items():
        setattr(c, k, v)
    h = ctypes.c_void_p()
    rc = _lib.lib().fg_edm2_create(ctypes.byref(c), ctypes.byref(h))
    return rc, h


def test_param_info_order():
    rc, h = _handle(D.IN64_S)
    assert rc == 0
    L = _lib.lib()
    try:
        name, nd, shp = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 4)()
        got = []
        for i in range(L.fg_edm2_num_params(h)):
            _lib.check(L.fg_edm2_param_info(h, i, ctypes.byref(name), ctypes.byref(nd), shp))
            got.append((name.value.decode(), tuple(shp[j] for j in range(nd.value))))
        # every entry but the host-side logvar head, in the reference's order
        assert got == [kv for kv in recorded_keys() if not kv[0].startswith("logvar_")]
        assert L.fg_edm2_param_info(h, len(got), ctypes.byref(name), ctypes.byref(nd), shp) == 1
    finally:
        L.fg_edm2_destroy(h)


@pytest.mark.parametrize("over,msg", [
    (dict(img_resolution=128), "img_resolution"),
    (dict(img_resolution=4, num_levels=1), "img_resolution"),
    (dict(model_channels=48), "multiple of 64"),
    (dict(compute_dtype=_lib.FG_DTYPE_F32), "compute_dtype"),
    (dict(img_channels=5), "img_channels"),
])
def test_create_envelope_refusals(over, msg):
    rc, h = _handle(**over)
    assert rc == 1 and h.value is None
    assert msg in _lib.lib().fg_last_error().decode()


def test_create_refuses_attention_below_8():
    cfg = D.EDM2Config(img_resolution=16, model_channels=64, channel_mult=[1, 1], num_blocks=1, attn_resolutions=[4], label_dim=0)
    rc, _ = _handle(cfg)
    assert rc == 0  # no level at 4x4: the list entry never matches
    cfg = D.EDM2Config(img_resolution=8, model_channels=64, channel_mult=[1, 1], num_blocks=1, attn_resolutions=[8], label_dim=0)
    rc, _ = _handle(cfg)
    assert rc == 1 and "lowest resolution" in _lib.lib().fg_last_error().decode()


def test_block_info_matches_layout_and_run_block_refuses_bad_split():
    rc, h = _handle(D.NARROW)
    assert rc == 0
    L = _lib.lib()
    try:
        enc, dec, _, _, _ = D.layout(D.NARROW)
        blocks = enc + dec
        assert L.fg_edm2_num_blocks(h) == len(blocks)
        key, v = ctypes.c_char_p(), [ctypes.c_int() for _ in range(5)]
        for i, b in enumerate(blocks):
            _lib.check(L.fg_edm2_block_info(h, i, ctypes.byref(key), *(ctypes.byref(x) for x in v)))
            assert (key.value.decode(), *(x.value for x in v)) == (b.key, b.cin, b.cout, b.res_in, b.res_out, int(b.attn))
        assert L.fg_edm2_block_info(h, len(blocks), None, None, None, None, None, None) == 1
        # a wrong (c1, c2) split is refused before any weight is touched (nothing is bound or packed here)
        i = next(j for j, b in enumerate(blocks) if b.skip_c)
        b = blocks[i]
        dummy = ctypes.c_void_p(16)
        rc = L.fg_edm2_run_block(h, i, dummy, b.cin, dummy, 0, dummy, dummy, 1, None, 0, None)
        assert rc == 1 and "channel split" in L.fg_last_error().decode()
        rc = L.fg_edm2_run_block(h, i, dummy, b.cin - b.skip_c, dummy, b.skip_c, dummy, dummy, 1, None, 0, None)
        assert rc == 2  # the right split gets as far as the unpacked weights
        assert L.fg_edm2_workspace_bytes(h, 2) > 0
    finally:
        L.fg_edm2_destroy(h)
