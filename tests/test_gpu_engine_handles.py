"""When the four network wrappers hand their weights to their engines: a call with untouched weights binds nothing, the call after an
in-place update of one parameter binds what belongs to the changed group - every engine parameter for EDMPrecond and EDM2Precond (one
signature over all of them), the one group of an unwrapped (no FSDP2) DiT and CausalWan, which holds all of theirs too - and the output
then is that of a fresh module loaded with the updated state dict.  `fg_{family}_bind_param` of the loaded library is counted."""
import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks.DiT.network import DiT
from fastgen_amd.networks.EDM.network import EDMPrecond
from fastgen_amd.networks.EDM2.network import EDM2Precond
from fastgen_amd.networks.Wan.network_causal import CausalWan

pytestmark = pytest.mark.gpu

SONG = dict(img_resolution=32, img_channels=3, label_dim=10, sigma_shift=0.0, sigma_data=0.5, model_type="SongUNet", augment_dim=9,
            model_channels=128, channel_mult=[2, 2, 2], channel_mult_noise=1, embedding_type="positional", encoder_type="standard",
            decoder_type="standard", resample_filter=[1, 1], dropout=0.0, label_dropout=0, r_timestep=False, drop_precond=None)
EDM2 = dict(img_resolution=16, img_channels=3, label_dim=0, model_channels=64, channel_mult=[1, 2], num_blocks=1, attn_resolutions=[8])
WAN = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2, chunk_size=2, total_num_frames=6)


def _seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _unet_call(res):
    x, t = _seeded((2, 3, res, res), 1), torch.tensor([1.0, 2.5], dtype=torch.float64).cuda()
    return lambda net: net(x, t)


def _dit_call():
    x, t, cls = _seeded((3, 4, 32, 32), 1), torch.tensor([0.9, 0.5, 0.2]).cuda(), torch.tensor([1, 7, 999]).cuda()
    return lambda net: net(x, t, cls)


def _wan_call():
    x, t, text = _seeded((1, 16, 6, 8, 8), 1), torch.full((1,), 0.6, dtype=torch.float64).cuda(), _seeded((1, 16, 128), 2)
    return lambda net: net(x, t, condition=text, fwd_pred_type="flow", is_ar=False)


# family: (constructor, the call, the parameter updated in place, the names the engine binds - out of the module's state dict)
CASES = {
    "edm": (lambda: EDMPrecond(**SONG), lambda: _unet_call(32), "model.enc.32x32_block1.conv0.weight",
            lambda net: [n for n, _ in net.named_parameters()]),
    "edm2": (lambda: EDM2Precond(**EDM2), lambda: _unet_call(16), "unet.enc.16x16_conv.weight",
             lambda net: [k for k in net.state_dict() if k.startswith("unet.")]),  # (not the host-side logvar head)
    "dit": (lambda: DiT(hidden_size=384, depth=1, num_heads=6), _dit_call, "x_embedder.proj.weight", lambda net: list(net.state_dict())),
    "wan": (lambda: CausalWan(**WAN), _wan_call, "transformer.patch_embedding.weight",
            lambda net: [n for n, _ in net.named_parameters() if "logvar_linear" not in n]),
}


@pytest.mark.parametrize("family", list(CASES))
def test_rebinding_happens_exactly_when_weights_change(family, monkeypatch):
    make, make_call, touched, bound_names = CASES[family]
    L = _lib.lib()
    real, bound = getattr(L, f"fg_{family}_bind_param"), []

    def counted(h, name, p, n):
        bound.append(name.decode())
        return real(h, name, p, n)

    monkeypatch.setattr(L, f"fg_{family}_bind_param", counted)
    net = make()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in net.parameters():  # (the default initial values zero whole branches: every parameter carries signal here)
            p.copy_(0.05 * torch.randn(p.shape, generator=g))
    net = net.cuda().eval()
    call = make_call()
    with torch.inference_mode():
        first = call(net)
    assert torch.isfinite(first).all()
    want = sorted(bound_names(net))
    assert sorted(bound) == want  # the first call binds every engine parameter once
    del bound[:]
    with torch.inference_mode():
        again = call(net)
    assert bound == [] and torch.equal(again, first)  # (a)
    with torch.no_grad():
        dict(net.named_parameters())[touched].mul_(0.5)
    with torch.inference_mode():
        updated = call(net)
    assert sorted(bound) == want  # (b)
    assert not torch.equal(updated, first)
    monkeypatch.undo()
    fresh = make()
    fresh.load_state_dict(net.state_dict(), strict=True)
    fresh = fresh.cuda().eval()
    with torch.inference_mode():
        assert torch.equal(call(fresh), updated)  # (c)
