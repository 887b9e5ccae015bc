"""When the Wan wrappers hand a condition to the handle and when they do not: the text, the image-to-video condition, the first frame,
the VACE context and the VACE scales go to the library once per (tensor object, in-place version, shape) - a wrong rule either embeds a
condition again on every call (slow, silent) or keeps a stale one after an in-place edit (wrong, silent).  The library's `fg_wan_set_*`
entry points are counted on the loaded CDLL object, through the public wrappers on the two-block networks and fixtures of
test_gpu_wan_conditions.py (video [2, 16, 3, 8, 8], 37 text tokens, 65 image tokens)."""
import pytest
import torch

from fastgen_amd import _lib
from oracle import wan_ref as R
import wan_i2v_ref as I
from test_gpu_wan_conditions import KW, SHAPE, TL, _load, _randn, _ti2v, _vace

pytestmark = pytest.mark.gpu

TEXT, I2V, FF, CTX, SCALE = COUNTED = ("fg_wan_set_text", "fg_wan_set_i2v_cond", "fg_wan_set_first_frame", "fg_wan_set_vace_context",
                                       "fg_wan_set_vace_scale")


@pytest.fixture
def new_calls(monkeypatch):
    """new_calls(fn): run fn under no_grad; the number of calls it made to each counted entry point."""
    L, n = _lib.lib(), dict.fromkeys(COUNTED, 0)
    for name in COUNTED:
        def counting(*args, _f=getattr(L, name), _name=name):
            n[_name] += 1
            return _f(*args)
        monkeypatch.setattr(L, name, counting)

    def run(fn):
        before = dict(n)
        with torch.no_grad():
            fn()
        return {k: n[k] - before[k] for k in COUNTED}
    return run


def _t():
    return torch.tensor([0.7, 0.4]).cuda()


def _text(seed):
    return _randn(seed, SHAPE[0], 37, 128)


def test_wan_text(new_calls):
    from fastgen_amd.networks.Wan.network import Wan

    net = _load(Wan(**KW), R.random_state_dict(R.TINY, 91))
    x, t, text, neg = _randn(1, *SHAPE), _t(), _text(2), _text(3)
    assert new_calls(lambda: net(x, t, text))[TEXT] == 1
    assert new_calls(lambda: net(x, t, text))[TEXT] == 0
    text.mul_(1.0)  # (an in-place edit: the version moves)
    assert new_calls(lambda: net(x, t, text))[TEXT] == 1
    clone = text.clone()
    assert new_calls(lambda: net(x, t, clone))[TEXT] == 1
    assert new_calls(lambda: net.few_step_sample(x, clone, TL, sample_type="ode"))[TEXT] == 0
    assert new_calls(lambda: net.sample(x, clone, neg, num_steps=2, solver="euler"))[TEXT] == 1
    assert new_calls(lambda: net(x, t, clone))[TEXT] == 1  # (the stacked text was forgotten)
    assert new_calls(lambda: net.sample(x, clone, None, num_steps=2, solver="euler"))[TEXT] == 1  # (it forgets before setting)
    assert new_calls(lambda: net(x, t, clone))[TEXT] == 0  # (an unguided sample leaves the key in place)
    with torch.no_grad():
        next(p for name, p in net.named_parameters() if ".blocks.0." in name).add_(0)
    assert new_calls(lambda: net(x, t, clone))[TEXT] == 1  # (packing forgets the text)


def test_i2v_condition(new_calls):
    from fastgen_amd.networks.WanI2V.network import WanI2V

    net = _load(WanI2V(**KW, image_dim=I.TINY_IMAGE_DIM), I.random_state_dict(I.TINY, I.TINY_IMAGE_DIM, 94))
    x, t = _randn(1, *SHAPE), _t()
    image = lambda seed: _randn(seed, SHAPE[0], 65, I.TINY_IMAGE_DIM)  # noqa: E731
    cond = {"text_embeds": _text(2), "first_frame_cond": _randn(3, *SHAPE), "encoder_hidden_states_image": image(4)}
    neg = {"text_embeds": _text(5), "first_frame_cond": _randn(6, *SHAPE), "encoder_hidden_states_image": image(7)}
    steps = [(lambda: net(x, t, cond), 1), (lambda: net(x, t, cond), 0)]
    other = dict(cond, encoder_hidden_states_image=image(8))
    steps += [(lambda: net(x, t, other), 1)]
    no_image = {k: v for k, v in cond.items() if k != "encoder_hidden_states_image"}
    steps += [(lambda: net(x, t, no_image), 1), (lambda: net.sample(x, cond, neg, num_steps=2, solver="euler"), 1), (lambda: net(x, t, cond), 1)]
    for i, (fn, want) in enumerate(steps):
        got = new_calls(fn)
        assert (got[I2V], got[FF]) == (want, 0), (i, got)


def test_ti2v_first_frame(new_calls):
    net, own = _ti2v()
    x, t = _randn(1, *SHAPE), _t()
    cond = dict(own, text_embeds=_text(2))
    neg = {"text_embeds": _text(5), "first_frame_cond": _randn(6, SHAPE[0], 16, 1, *SHAPE[3:])}
    steps = [(lambda: net(x, t, cond), 1), (lambda: net(x, t, cond), 0)]
    # (a fresh frame-0 view or a fresh stack each time)
    steps += [(lambda: net.sample(x, cond, None, num_steps=2, solver="euler"), 1)] * 2 + [(lambda: net.sample(x, cond, neg, num_steps=2, solver="euler"), 1)] * 2
    for i, (fn, want) in enumerate(steps):
        got = new_calls(fn)
        assert (got[FF], got[I2V]) == (want, 0), (i, got)


def test_vace_context_and_scales(new_calls):
    net, own = _vace()
    x, t = _randn(1, *SHAPE), _t()
    cond = dict(own, text_embeds=_text(2))

    def step(c=cond):
        got = new_calls(lambda: net(x, t, c))
        return got[TEXT], got[CTX], got[SCALE]

    assert step() == (1, 1, 1)
    assert step() == (0, 0, 0)
    net.context_scale = 0.5
    assert step() == (0, 0, 1)
    other = dict(cond, vid_context=cond["vid_context"].clone())
    assert step(other) == (0, 1, 0)
    net._forget_text()
    assert step(other) == (1, 1, 0)


def test_causal_text_per_cache_tag(new_calls):
    from fastgen_amd.networks.Wan.network_causal import CausalWan

    net = CausalWan(**KW, chunk_size=1, total_num_frames=3).cuda().eval()
    video, t, a, b = _randn(1, *SHAPE), _t(), _text(2), _text(3)
    x = video[:, :, :1].contiguous()
    fwd = lambda tag, text: new_calls(lambda: net(x, t, text, is_ar=True, cache_tag=tag))[TEXT]  # noqa: E731
    assert fwd("pos", a) == 1
    assert fwd("neg", b) == 1
    assert fwd("pos", a) == 0
    assert fwd("neg", b) == 0
    net.clear_caches()
    assert fwd("pos", a) == 1
    assert new_calls(lambda: net.student_sample(video.clone(), TL, a, sample_type="ode"))[TEXT] == 0  # (tag "pos" holds A already)
    assert fwd("pos", a) == 1  # (the loop ends with clear_caches(): the text is forgotten with them)
