"""The handle-owned condition buffers of the bidirectional video DiT across calls that reallocate them (the text's k / v per block,
the image tokens and their k / v, the first frame, the VACE context): a loop's graph names these buffers, the allocator may hand a
freed address out again, so a call after a reallocation must capture anew and still equal the eager call.  Through the Python
wrappers on the two-block networks of the Wan tests (2 heads, D 256, ffn 512, text_dim 128), video [2, 16, 3, 8, 8] (48 tokens per
sample).  Equality tests of correct calls: bit-equal to `use_graph=False`, capture counts from `_lib.graph_stats()`."""
import pytest
import torch

from fastgen_amd import _lib
from oracle import wan_ref as R
import wan_i2v_ref as I
import wan_ti2v_ref as T
import wan_vace_ref as V

pytestmark = pytest.mark.gpu

KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2)
SHAPE = (2, 16, 3, 8, 8)
TL = [0.999, 0.6, 0.25, 0.0]
TEXT_LENS = (37, 21, 37)


def _load(net, sd):
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _graph_and_eager(call):
    """call(use_graph) twice: (the graph call's result, the graphs it captured); the result is finite and bit-equal to the eager
    call's, which captures nothing."""
    c0 = _lib.graph_stats()[0]
    with torch.inference_mode():
        got = call(True)
        captures = _lib.graph_stats()[0] - c0
        want = call(False)
    assert _lib.graph_stats()[0] - c0 == captures, "the eager call captured a graph"
    assert torch.isfinite(got).all() and torch.equal(got, want)
    return got, captures


@pytest.mark.parametrize("loop", ["few_step_sample", "sample"])
def test_text_of_three_lengths(loop):
    """37 tokens, 21, 37 again: every block's text k / v buffer is reallocated before each call, each call captures its one graph."""
    from fastgen_amd.networks.Wan.network import Wan

    net = _load(Wan(**KW), R.random_state_dict(R.TINY, 91))
    noise = _randn(92, *SHAPE)
    texts = {n: (_randn(93 + n, SHAPE[0], n, 128), _randn(193 + n, SHAPE[0], n, 128)) for n in set(TEXT_LENS)}
    results = []
    for n in TEXT_LENS:
        cond, neg = texts[n]
        if loop == "few_step_sample":
            got, captures = _graph_and_eager(lambda g: net.few_step_sample(noise, cond, TL, sample_type="ode", use_graph=g))
        else:
            got, captures = _graph_and_eager(lambda g: net.sample(noise, cond, neg, num_steps=2, solver="euler", use_graph=g))
        assert captures == 1, (n, captures)
        results.append(got)
    assert torch.equal(results[2], results[0]) and not torch.equal(results[1], results[0])


def test_image_tokens_of_three_lengths_then_new_contents():
    """65 image tokens, 33, 65 again at one video shape (96, 64, 96 padded rows: the image tokens and every block's image k / v are
    reallocated), one capture per call; then new image contents at 65: the buffers stay, so does the graph."""
    from fastgen_amd.networks.WanI2V.network import WanI2V

    net = _load(WanI2V(**KW, image_dim=I.TINY_IMAGE_DIM), I.random_state_dict(I.TINY, I.TINY_IMAGE_DIM, 94))
    noise = _randn(95, *SHAPE)
    cond = {"text_embeds": _randn(96, SHAPE[0], 37, 128), "first_frame_cond": _randn(97, *SHAPE)}
    images = {n: _randn(98 + n, SHAPE[0], n, I.TINY_IMAGE_DIM) for n in (65, 33)}

    def run(image):
        c = dict(cond, encoder_hidden_states_image=image)
        return _graph_and_eager(lambda g: net.few_step_sample(noise, c, TL, sample_type="ode", use_graph=g))

    results = []
    for n in (65, 33, 65):
        got, captures = run(images[n])
        assert captures == 1, (n, captures)
        results.append(got)
    assert torch.equal(results[2], results[0]) and not torch.equal(results[1], results[0])
    got, captures = run(_randn(99, SHAPE[0], 65, I.TINY_IMAGE_DIM))
    assert captures == 0 and not torch.equal(got, results[0])


def _ti2v():
    from fastgen_amd.networks.WanI2V.network import WanI2V

    net = WanI2V(**KW, concat_mask=False, use_image_encoder=False, expand_timesteps=True, image_dim=None, in_channels=16, out_channels=16)
    return _load(net, T.random_state_dict(R.TINY, 101)), {"first_frame_cond": _randn(102, SHAPE[0], 16, 1, *SHAPE[3:])}


def _vace():
    from fastgen_amd.networks.VaceWan.network import VACEWan

    net = VACEWan(**KW, vace_layers=(0, 1), context_scale=V.SCALES)
    return _load(net, V.random_state_dict(R.TINY, 103, vace_layers=(0, 1))), {"vid_context": _randn(104, SHAPE[0], V.VACE_IN, *SHAPE[2:])}


@pytest.mark.parametrize("make", [_ti2v, _vace], ids=["ti2v", "vace"])
def test_condition_for_batch_two_then_one_then_two(make):
    """The first frame / the VACE context (and the text) set for batch 2, the network then called at batch 1 and at batch 2 again: the
    buffers are reallocated twice, the last call is the first one bit for bit."""
    net, own = make()
    noise = _randn(105, *SHAPE)
    cond2 = dict(own, text_embeds=_randn(106, SHAPE[0], 37, 128))
    cond1 = {k: v[:1].contiguous() for k, v in cond2.items()}

    def run(x, c):
        return _graph_and_eager(lambda g: net.few_step_sample(x, c, TL, sample_type="ode", use_graph=g))[0]

    first = run(noise, cond2)
    one = run(noise[:1].contiguous(), cond1)
    assert one.shape[0] == 1
    again = run(noise, cond2)
    assert torch.equal(again, first)
