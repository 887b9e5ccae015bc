"""The two up-sampling UNetBlocks (8 -> 16 and 16 -> 32, 256 -> 256 channels) of the EDM CIFAR-10 U-Net in the split-bf16 mode,
whose inference forward runs conv0 as four 2x2 convolutions on the low-resolution input (conv_ws3.hip, RES_SUBPIX: per output
phase the 3x3 kernel's rows / columns that read the same replicated pixel are merged at pack time) and the 1x1 skip once per
low-resolution pixel, conv1 fetching its residual at (y >> 1, x >> 1).

Checked: each block against the fp64 restatement at the bf16x3 parity bound of tests/test_gpu_parity.py (B = 1, 3, 16; 3 leaves the
last image pair of the 8x8-source geometry half empty); the same with weights whose nine taps have very different sizes and a
distinct value per input pixel, where a reference with ONE phase merged wrongly is shown to miss the bound by orders of magnitude;
the low-resolution skip alone bit-equal to the full-resolution launches; every image independent of its batch mates bit for bit;
one forward and the 4-step sampler against the recorded reference outputs, graph replay bit-equal to eager launches.

FASTGEN_AMD_CONV_SUBPIX is read once per process, so the other settings of the switch run in child processes (this file as a
script), one per setting, shared by the tests that need them."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # run as a script (the child processes below)
    sys.path.insert(0, ROOT)

import pytest
import torch
import torch.nn.functional as F

from fastgen_amd import _lib
from fastgen_amd.methods.model import FastGenModel
from fastgen_amd.networks.EDM.network import EDMPrecond
from oracle import edm_ref as R

pytestmark = pytest.mark.gpu

KW = dict(img_resolution=32, img_channels=3, label_dim=10, sigma_shift=0.0, sigma_data=0.5, model_type="SongUNet",
          augment_dim=9, model_channels=128, channel_mult=[2, 2, 2], channel_mult_noise=1, embedding_type="positional",
          encoder_type="standard", decoder_type="standard", resample_filter=[1, 1], dropout=0.0, label_dropout=0,
          r_timestep=False, drop_precond=None)
MAX_ABS, REL = 5e-5, 2e-5  # the bf16x3 block bound of tests/test_gpu_parity.py
BIG = 16                   # the largest batch; the smaller ones are its leading images


def dev():
    return torch.device("cuda:0")


def up_blocks():
    enc, dec = R.layout(R.CIFAR10)
    blocks = [b for b in enc + dec if b.kind == "block"]
    return [(i, b) for i, b in enumerate(blocks) if b.up]


def make_net(sd):
    n = EDMPrecond(compute_dtype="bf16x3", **KW)
    n.load_state_dict(sd, strict=True)
    return n.to(dev()).eval()


def run_block(net, index, b, x, emb):
    """fg_edm_run_block on NCHW fp32 x (CPU); returns the NCHW output (CPU)."""
    L = _lib.lib()
    bs = x.shape[0]
    x1 = x.permute(0, 2, 3, 1).contiguous().to(dev())
    e = emb.to(dev()).contiguous()
    out = torch.empty(bs, b.res, b.res, b.cout, device=dev())
    dt, h = net._engine(dev())
    ws = net._workspace(dt, h, bs, dev())
    _lib.check(L.fg_edm_run_block(h, index, x1.data_ptr(), b.cin, None, 0, e.data_ptr(), out.data_ptr(), bs, ws.data_ptr(),
                                  ws.numel(), None))
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).contiguous().cpu()


def inputs(b, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(BIG, b.cin, b.res // 2, b.res // 2, generator=g)
    emb = torch.randn(BIG, R.CIFAR10.emb_channels, generator=g)
    return x, emb


def errors(got, want):
    return (got - want).abs().max().item(), ((got - want).norm() / want.norm()).item()


@pytest.fixture(scope="module")
def sd():
    return R.random_state_dict(R.CIFAR10, seed=1234)


@pytest.fixture(scope="module")
def net(sd):
    return make_net(sd)


@pytest.fixture(scope="module")
def cases(sd):
    """Per up block: inputs of the largest batch and their fp64 reference (GroupNorm is per image: any leading part of the batch
    has the leading part of the reference)."""
    sd64 = {k: v.double() for k, v in sd.items()}
    out = {}
    with torch.inference_mode():
        for index, b in up_blocks():
            x, emb = inputs(b, 300 + index)
            out[index] = (b, x, emb, R.unet_block(sd64, b, x.double(), emb.double()).float())
    return out


@pytest.fixture(scope="module")
def big(net, cases):
    """The blocks' outputs at the largest batch."""
    with torch.inference_mode():
        return {index: run_block(net, index, b, x, emb) for index, (b, x, emb, _) in cases.items()}


def test_layout_has_the_two_up_blocks():
    assert [(b.cin, b.cout, b.res, b.skip_from) for _, b in up_blocks()] == [(256, 256, 16, None), (256, 256, 32, None)]


# ---- case 1: each block against fp64 -------------------------------------------------------------------------------


@pytest.mark.parametrize("bs", [1, 3, 16])
def test_up_blocks_against_fp64(net, cases, big, bs):
    with torch.inference_mode():
        for index, (b, x, emb, want) in cases.items():
            got = big[index] if bs == BIG else run_block(net, index, b, x[:bs].contiguous(), emb[:bs].contiguous())
            assert torch.isfinite(got).all(), b.key
            err, rel = errors(got, want[:bs])
            print(f"{b.key} B={bs}: max_abs={err:.3e} rel_l2={rel:.3e}")
            assert err <= MAX_ABS and rel <= REL, f"{b.key} B={bs}: max_abs={err:.3e} rel_l2={rel:.3e}"


# ---- case 2: phase and border sensitivity --------------------------------------------------------------------------

# rows / columns of the 3x3 kernel that read the same low-resolution pixel, per output parity and merged tap
MERGE = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}


def subpixel_conv(x, w, bias, wrong_phase=None):
    """conv3x3(nearest_up2(x)) restated as four 2x2 convolutions on x (any dtype), the way the kernel evaluates it.  wrong_phase:
    that output phase (py, px) takes the column merge of the OTHER column parity, a mis-packed weight block."""
    B, C, H, W = x.shape
    out = x.new_zeros(B, w.shape[0], 2 * H, 2 * W)
    xp = F.pad(x, (1, 1, 1, 1))
    for py in (0, 1):
        for px in (0, 1):
            cols = MERGE[1 - px] if wrong_phase == (py, px) else MERGE[px]
            w2 = torch.stack([torch.stack([w[:, :, list(MERGE[py][ty])][:, :, :, list(cols[tx])].sum(dim=(2, 3)) for tx in (0, 1)], dim=-1)
                              for ty in (0, 1)], dim=-2)  # [co, ci, ty, tx]
            # tap (ty, tx) reads padded pixel (y + py + ty, x + px + tx): a valid 2x2 conv of the window starting at (py, px)
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], w2)
    return out + bias.reshape(1, -1, 1, 1)


def block_with_conv0(sd, b, x, emb, conv0):
    """R.unet_block of an up block without attention, conv0 supplied by the caller."""
    k = b.key
    h = F.silu(R.group_norm(x, sd[f"{k}.norm0.weight"], sd[f"{k}.norm0.bias"], R.BLOCK_EPS))
    h = conv0(h, sd[f"{k}.conv0.weight"], sd[f"{k}.conv0.bias"])
    h = h + R.linear(emb, sd[f"{k}.affine.weight"], sd[f"{k}.affine.bias"])[:, :, None, None]
    h = F.silu(R.group_norm(h, sd[f"{k}.norm1.weight"], sd[f"{k}.norm1.bias"], R.BLOCK_EPS))
    h = R.conv2d(h, sd[f"{k}.conv1.weight"], sd[f"{k}.conv1.bias"])
    skip = R.conv2d(x, sd[f"{k}.skip.weight"], sd[f"{k}.skip.bias"], up=True)
    return (h + skip) * R.SKIP_SCALE


def test_phase_and_border_sensitivity(sd):
    """conv0 weights whose nine taps differ in size by up to 5x (the overall scale keeps the output O(1)) and an input that adds a
    distinct offset per pixel to the noise: a wrong phase -> window mapping or a wrong merged tap cannot cancel.  The reference
    with one mis-packed phase misses the bound by the factor printed (measured: see the assertion message of a failing run; the
    assertion asks for two orders of magnitude)."""
    tap = torch.tensor([[0.4, 1.0, 1.6], [2.0, 0.6, 1.2], [0.8, 1.8, 1.4]])
    sd2 = dict(sd)
    for _, b in up_blocks():
        sd2[f"{b.key}.conv0.weight"] = sd[f"{b.key}.conv0.weight"] * tap / tap.square().mean().sqrt()
    net2 = make_net(sd2)
    sd64 = {k: v.double() for k, v in sd2.items()}
    bs = 2
    with torch.inference_mode():
        for index, b in up_blocks():
            r = b.res // 2
            g = torch.Generator().manual_seed(400 + index)
            ramp = torch.linspace(-1.0, 1.0, r * r).reshape(1, 1, r, r)
            x = torch.randn(bs, b.cin, r, r, generator=g) + ramp
            emb = torch.randn(bs, R.CIFAR10.emb_channels, generator=g)
            got = run_block(net2, index, b, x, emb)
            want = R.unet_block(sd64, b, x.double(), emb.double())
            # the restatement itself is exact, and is what the reference computes
            same = block_with_conv0(sd64, b, x.double(), emb.double(), subpixel_conv)
            assert (same - want).abs().max().item() < 1e-10
            err, rel = errors(got, want.float())
            print(f"{b.key}: max_abs={err:.3e} rel_l2={rel:.3e}")
            assert err <= MAX_ABS and rel <= REL, f"{b.key}: max_abs={err:.3e} rel_l2={rel:.3e}"
            for wrong in ((0, 1), (1, 0)):
                bad = block_with_conv0(sd64, b, x.double(), emb.double(), lambda h, w, c: subpixel_conv(h, w, c, wrong_phase=wrong))
                berr, brel = errors(got, bad.float())
                print(f"{b.key}: phase {wrong} mis-packed in the reference: max_abs={berr:.3e} ({berr / MAX_ABS:.0f}x the bound) "
                      f"rel_l2={brel:.3e} ({brel / REL:.0f}x)")
                assert berr > 100 * MAX_ABS and brel > 100 * REL, (b.key, wrong, berr, brel)


# ---- case 3: the low-resolution skip alone is exact; the switch --------------------------------------------------------


def dump(path):
    """Child process: the blocks' outputs at B = 3 under this process's FASTGEN_AMD_CONV_SUBPIX."""
    sd_ = R.random_state_dict(R.CIFAR10, seed=1234)
    net_ = make_net(sd_)
    out = {}
    with torch.inference_mode():
        for index, b in up_blocks():
            x, emb = inputs(b, 300 + index)
            out[index] = run_block(net_, index, b, x[:3].contiguous(), emb[:3].contiguous())
    torch.save(out, path)


@pytest.fixture(scope="module")
def by_switch(tmp_path_factory):
    got = {}
    for value in ("0", "skip"):
        path = str(tmp_path_factory.mktemp("subpix") / f"blocks_{value}.pt")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, FASTGEN_AMD_CONV_SUBPIX=value),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[value] = torch.load(path, weights_only=True)
    return got


def test_low_resolution_skip_is_exact(by_switch):
    """A 1x1 conv commutes with nearest replication product for product: with only the skip moved to the low resolution the block
    output equals the full-resolution launches' bit for bit."""
    for index, b in up_blocks():
        assert torch.equal(by_switch["skip"][index], by_switch["0"][index]), b.key


def test_switch_selects_the_launches(net, cases, by_switch):
    """FASTGEN_AMD_CONV_SUBPIX=0 keeps the replicated 3x3 (same bound against fp64); the default takes the merged weights, whose
    rounding differs from it somewhere (an equal output would mean the new path never ran)."""
    active = os.environ.get("FASTGEN_AMD_CONV_SUBPIX", "1")[:1] not in ("0", "s") and os.environ.get("FASTGEN_AMD_CONV_WS", "1")[:1] != "0"
    with torch.inference_mode():
        for index, (b, x, emb, want) in cases.items():
            err, rel = errors(by_switch["0"][index], want[:3])
            assert err <= MAX_ABS and rel <= REL, f"{b.key} (switch off): max_abs={err:.3e} rel_l2={rel:.3e}"
            got = run_block(net, index, b, x[:3].contiguous(), emb[:3].contiguous())
            assert not active or not torch.equal(got, by_switch["0"][index]), b.key
            assert (got - by_switch["0"][index]).abs().max().item() <= 2 * MAX_ABS


# ---- case 4: batch invariance --------------------------------------------------------------------------------------


def test_up_blocks_batch_independent(net, cases, big):
    with torch.inference_mode():
        for index, (b, x, emb, _) in cases.items():
            for lo, n in ((0, 1), (15, 1), (0, 5), (11, 5)):
                small = run_block(net, index, b, x[lo:lo + n].contiguous(), emb[lo:lo + n].contiguous())
                assert torch.equal(big[index][lo:lo + n], small), f"{b.key}: rows {lo}..{lo + n - 1} depend on the batch"


# ---- case 5: whole network -----------------------------------------------------------------------------------------


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def check(got, want, what):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert torch.isfinite(got).all(), what
    err, rel = errors(got, want)
    print(f"{what}: max_abs={err:.3e} rel_l2={rel:.3e}")
    assert err <= MAX_ABS and rel <= REL, f"{what}: max_abs={err:.3e} rel_l2={rel:.3e}"


def test_forward_and_sampler_against_reference_golden(net, golden_dir):
    fx = torch.load(os.path.join(golden_dir, "forward_full_b2.pt"), weights_only=True)
    x = (seeded((2, 3, 32, 32), 21) * fx["t"].reshape(2, 1, 1, 1).float()).to(dev())
    with torch.inference_mode():
        out = net(x, fx["t"].to(dev()), condition=fx["cond"].to(dev()), fwd_pred_type="x0")
    check(out, fx["out"], "EDMPrecond.forward B=2")
    fx = torch.load(os.path.join(golden_dir, "sampler_full_b2.pt"), weights_only=True)
    noise = seeded((2, 3, 32, 32), 0).to(dev())
    cond = fx["cond"].to(dev())
    eps = torch.stack([seeded((2, 3, 32, 32), s) for s in (1, 2, 3)]).to(dev())
    gf = FastGenModel.generator_fn
    sde = gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="sde", eps=eps)
    check(sde, fx["out_sde"], "4-step sde (graph)")
    eager = gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="sde", eps=eps, use_graph=False)
    assert torch.equal(sde, eager), "graph replay and eager launches must agree bit for bit"
    assert torch.equal(sde, gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="sde", eps=eps))


if __name__ == "__main__":
    dump(sys.argv[1])
