"""The 16x16 single-head attention blocks of the EDM CIFAR-10 U-Net in the bf16x3 mode with their weights merged at pack time
(engine.hip run_block, attn.hip): q' = (Wk^T Wq) xn + Wk^T bq, keys = xn = GroupNorm2(x) itself, v' = (Wp Wv) xn + Wp bv, and the
attention kernel's store applies proj.bias, the residual, sqrt(1/2) and the output's GroupNorm statistics.

Every case uses a state dict whose qkv.bias, proj.bias and norm2 weight / bias are seeded N(0, 1): with the (near) zero biases of
the default random state dict every bias term of the derivation would vanish.  Blocks are checked against oracle.edm_ref.unet_block
in fp64 at the bf16x3 block tolerance of tests/test_gpu_edm_step.py; the whole forward at the bf16x3 tolerance of
tests/test_gpu_parity.py (it is what reads the statistics slots the new epilogue writes: the next block's norm0)."""
import os
import subprocess
import sys

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks.EDM.network import EDMPrecond
from oracle import edm_ref as R

gpu = pytest.mark.gpu

KW = dict(img_resolution=32, img_channels=3, label_dim=10, sigma_shift=0.0, sigma_data=0.5, model_type="SongUNet",
          augment_dim=9, model_channels=128, channel_mult=[2, 2, 2], channel_mult_noise=1, embedding_type="positional",
          encoder_type="standard", decoder_type="standard", resample_filter=[1, 1], dropout=0.0, label_dropout=0,
          r_timestep=False, drop_precond=None)
MAX_ABS, REL = 5e-5, 2e-5  # tests/test_gpu_edm_step.py; the bf16x3 forward tolerance of tests/test_gpu_parity.py is the same pair


def dev():
    return torch.device("cuda:0")


def attn_blocks_16():
    """(index among the UNetBlocks, spec) of every 16x16 attention block: four in the encoder, one in the decoder (256 + 256 concat)."""
    enc, dec = R.layout(R.CIFAR10)
    blocks = [b for b in enc + dec if b.kind == "block"]
    return [(i, b) for i, b in enumerate(blocks) if b.res == 16 and b.attn]


def biased_state_dict():
    sd = R.random_state_dict(R.CIFAR10, seed=1234)
    g = torch.Generator().manual_seed(4321)
    for k in sorted(sd):
        if k.endswith((".qkv.bias", ".proj.bias", ".norm2.weight", ".norm2.bias")):
            sd[k] = torch.randn(sd[k].shape, generator=g)
    return sd


@pytest.fixture(scope="module")
def sd():
    return biased_state_dict()


def make_net(state):
    n = EDMPrecond(compute_dtype="bf16x3", **KW)
    n.load_state_dict(state, strict=True)
    return n.to(dev()).eval()


@pytest.fixture(scope="module")
def net(sd):
    return make_net(sd)


def run_block(net, index, b, x, emb):
    """fg_edm_run_block on NCHW fp32 x (CPU); returns the NCHW output (CPU)."""
    L = _lib.lib()
    bs = x.shape[0]
    c2 = b.skip_from or 0
    c1 = b.cin - c2
    x1 = x[:, :c1].permute(0, 2, 3, 1).contiguous().to(dev())
    x2 = x[:, c1:].permute(0, 2, 3, 1).contiguous().to(dev()) if c2 else None
    e = emb.to(dev()).contiguous()
    out = torch.empty(bs, b.res, b.res, b.cout, device=dev())
    dt, h = net._engine(dev())
    ws = net._workspace(dt, h, bs, dev())
    _lib.check(L.fg_edm_run_block(h, index, x1.data_ptr(), c1, x2.data_ptr() if c2 else None, c2, e.data_ptr(), out.data_ptr(),
                                  bs, ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).contiguous().cpu()


def inputs(b, bs, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(bs, b.cin, b.res, b.res, generator=g)
    emb = torch.randn(bs, R.CIFAR10.emb_channels, generator=g)
    return x, emb


def oracle_block(state, b, x, emb):
    sd64 = {k: v.double() for k, v in state.items() if k.startswith(b.key + ".")}
    with torch.inference_mode():
        return R.unet_block(sd64, b, x.double(), emb.double()).float()


def assert_parity(got, want, what):
    assert torch.isfinite(got).all(), what
    err = (got - want).abs().max().item()
    rel = ((got - want).norm() / want.norm()).item()
    print(f"{what}: max_abs={err:.3e} rel_l2={rel:.3e}")
    assert err <= MAX_ABS and rel <= REL, f"{what}: max_abs={err:.3e} rel_l2={rel:.3e}"


def test_layout_has_five_16x16_attention_blocks():
    got = [(b.cin, b.skip_from or 0, b.cout) for _, b in attn_blocks_16()]
    assert sorted(got) == [(256, 0, 256)] * 4 + [(512, 256, 256)]


def merged_attention(state, key, x):
    """The block's attention half from the merged weights, in the dtype of x: x -> (proj(attention(qkv(norm2(x)))) + x) * sqrt(1/2)."""
    dt = x.dtype
    C = x.shape[1]
    wqkv = state[f"{key}.qkv.weight"].to(dt).reshape(C, 3, C)  # row c * 3 + plane
    bqkv = state[f"{key}.qkv.bias"].to(dt).reshape(C, 3)
    wq, wk, wv = wqkv[:, 0], wqkv[:, 1], wqkv[:, 2]
    bq, bv = bqkv[:, 0], bqkv[:, 2]  # bk drops out: q_i . bk is the same for every key
    wp, bp = state[f"{key}.proj.weight"].to(dt).reshape(C, C), state[f"{key}.proj.bias"].to(dt)
    m_q, c_q = wk.t() @ wq, wk.t() @ bq
    m_v, c_v = wp @ wv, wp @ bv
    xn = R.group_norm(x, state[f"{key}.norm2.weight"], state[f"{key}.norm2.bias"], R.BLOCK_EPS).flatten(2)  # [B][C][T]
    qm = torch.einsum("oi,bit->bot", m_q, xn) + c_q[None, :, None]
    vm = torch.einsum("oi,bit->bot", m_v, xn) + c_v[None, :, None]
    p = (torch.einsum("bcq,bck->bqk", qm, xn) / C ** 0.5).softmax(dim=2)
    o = torch.einsum("bqk,bck->bcq", p, vm) + bp[None, :, None]
    return (o.reshape(x.shape) + x) * R.SKIP_SCALE


def test_merge_formulas_reproduce_the_oracle_in_fp64(sd):
    """No GPU: pins the c * 3 + plane row order and which bias goes where.  The oracle's attention rounds q and k to fp32 for the
    logits (the reference's AttentionOp), so it is evaluated here with that cast made a no-op; everything else is unet_block itself."""
    _, b = attn_blocks_16()[1]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, b.cout, b.res, b.res, generator=g, dtype=torch.float64)
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith(b.key + ".")}
    k = b.key
    qkv = R.conv2d(R.group_norm(x, sd64[f"{k}.norm2.weight"], sd64[f"{k}.norm2.bias"], R.BLOCK_EPS), sd64[f"{k}.qkv.weight"], sd64[f"{k}.qkv.bias"])
    B, C3, H, W = qkv.shape
    q, kk, v = qkv.reshape(B, C3 // 3, 3, H * W).unbind(2)
    w = torch.einsum("ncq,nck->nqk", q, kk / (C3 // 3) ** 0.5).softmax(dim=2)
    a = torch.einsum("nqk,nck->ncq", w, v).reshape(B, C3 // 3, H, W)
    want = (R.conv2d(a, sd64[f"{k}.proj.weight"], sd64[f"{k}.proj.bias"]) + x) * R.SKIP_SCALE
    # the same thing through the oracle's own attention(), whose fp32 logits bound the agreement at fp32 level
    want32 = (R.conv2d(R.attention(qkv), sd64[f"{k}.proj.weight"], sd64[f"{k}.proj.bias"]) + x) * R.SKIP_SCALE
    assert ((want32 - want).norm() / want.norm()).item() < 1e-5
    got = merged_attention(sd64, k, x)
    rel = ((got - want).norm() / want.norm()).item()
    assert rel <= 1e-12, rel
    # a wrong row order (plane * C + c) or swapped biases must not pass
    bad = dict(sd64)
    bad[f"{k}.qkv.bias"] = sd64[f"{k}.qkv.bias"].reshape(3, -1).t().reshape(-1)
    assert ((merged_attention(bad, k, x) - want).norm() / want.norm()).item() > 1e-3


@gpu
@pytest.mark.parametrize("bs", [1, 3, 16])
def test_attn_blocks_against_fp64(net, sd, bs):
    for index, b in attn_blocks_16():
        x, emb = inputs(b, bs, 300 + index)
        with torch.inference_mode():
            got = run_block(net, index, b, x, emb)
        assert_parity(got, oracle_block(sd, b, x, emb), f"{b.key} B={bs}")


@gpu
def test_large_key_bias_cancels(sd):
    """bk x 30: q . bk is hundreds of logits, constant along each softmax row; fp64 cancels it, the merged path never forms it."""
    index, b = attn_blocks_16()[2]
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2[f"{b.key}.qkv.bias"][1::3] *= 30.0
    x, emb = inputs(b, 3, 400)
    n = make_net(sd2)
    with torch.inference_mode():
        got = run_block(n, index, b, x, emb)
    assert_parity(got, oracle_block(sd2, b, x, emb), f"{b.key} bk x 30")


@gpu
def test_batch_independent(net):
    """Images 1..2 of a B = 5 launch equal the same images run as B = 2, bit for bit."""
    with torch.inference_mode():
        for index, b in attn_blocks_16():
            x, emb = inputs(b, 5, 500 + index)
            big = run_block(net, index, b, x, emb)
            small = run_block(net, index, b, x[1:3].contiguous(), emb[1:3].contiguous())
            assert torch.equal(big[1:3], small), f"{b.key}: images 1..2 depend on the batch"


@gpu
def test_repack_after_in_place_update(sd):
    """qkv.weight and proj.weight multiplied in place: the merged copies must follow.  Stale merged weights would give the output of
    the old weights, which misses the new oracle by the factor asserted below (computed on the CPU from the oracle)."""
    index, b = attn_blocks_16()[0]
    n = make_net(sd)
    x, emb = inputs(b, 2, 600)
    want_old = oracle_block(sd, b, x, emb)
    with torch.inference_mode():
        assert_parity(run_block(n, index, b, x, emb), want_old, f"{b.key} before the update")
    g = torch.Generator().manual_seed(77)
    params = dict(n.named_parameters())
    sd2 = {k: v.clone() for k, v in sd.items()}
    with torch.no_grad():
        for name in (f"{b.key}.qkv.weight", f"{b.key}.proj.weight"):
            f = 0.5 + torch.rand(sd[name].shape, generator=g)
            params[name].mul_(f.to(dev()))
            sd2[name] = sd[name] * f
    want_new = oracle_block(sd2, b, x, emb)
    stale = (want_old - want_new).abs().max().item()
    print(f"stale merged weights would miss by max_abs={stale:.3e}")
    assert stale > 1000 * MAX_ABS
    with torch.inference_mode():
        assert_parity(run_block(n, index, b, x, emb), want_new, f"{b.key} after the update")


@gpu
def test_three_launch_path_still_passes():
    """FASTGEN_AMD_ATTN_MERGE=0 (read once per process, so in a child process): the q|k|v conv, attention and proj launches."""
    if os.environ.get("FASTGEN_AMD_ATTN_MERGE") == "0":
        pytest.skip("already running without the merged path")
    env = dict(os.environ, FASTGEN_AMD_ATTN_MERGE="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__) + "::test_attn_blocks_against_fp64[1]", "-q", "-x", "-m", "gpu"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@gpu
def test_whole_forward_against_oracle(net, sd):
    B = 3
    g = torch.Generator().manual_seed(9)
    x, t = torch.randn(B, 3, 32, 32, generator=g) * 2, torch.full((B,), 2.5265, dtype=torch.float64)
    cond = torch.nn.functional.one_hot(torch.arange(B) % 10, 10).float()
    with torch.inference_mode():
        want = R.edm_precond_forward(sd, R.CIFAR10, x, t, cond)
        got = net(x.to(dev()), t.to(dev()), condition=cond.to(dev())).float().cpu()
    assert_parity(got, want.float(), "forward B=3")
