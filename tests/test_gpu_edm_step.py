"""The 8x8 layers of the EDM CIFAR-10 U-Net on the split-bf16 wave-specialised 3x3 kernel (conv_ws3.hip, two whole 8x8 images
per 8x16 tile): every 8x8 UNetBlock against an fp64 CPU restatement at the bf16x3 parity tolerance (tests/test_gpu_parity.py),
at batches that fill the image pairs and ones that leave the last pair half empty, with the concatenated decoder inputs; each image
bit-exact independent of its batch mates at B = 512; and the same checks through the generic kernel (FASTGEN_AMD_CONV_WS=0)."""
import os
import subprocess
import sys

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks.EDM.network import EDMPrecond
from oracle import edm_ref as R

pytestmark = pytest.mark.gpu

KW = dict(img_resolution=32, img_channels=3, label_dim=10, sigma_shift=0.0, sigma_data=0.5, model_type="SongUNet",
          augment_dim=9, model_channels=128, channel_mult=[2, 2, 2], channel_mult_noise=1, embedding_type="positional",
          encoder_type="standard", decoder_type="standard", resample_filter=[1, 1], dropout=0.0, label_dropout=0,
          r_timestep=False, drop_precond=None)
MAX_ABS, REL = 5e-5, 2e-5  # the bf16x3 tolerance of tests/test_gpu_parity.py


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return R.random_state_dict(R.CIFAR10, seed=1234)


@pytest.fixture(scope="module")
def net(sd):
    n = EDMPrecond(compute_dtype="bf16x3", **KW)
    n.load_state_dict(sd, strict=True)
    return n.to(dev()).eval()


def blocks_8x8():
    enc, dec = R.layout(R.CIFAR10)
    blocks = [b for b in enc + dec if b.kind == "block"]
    return [(i, b) for i, b in enumerate(blocks) if b.res == 8]


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
    res_in = b.res * 2 if b.down else b.res
    x = torch.randn(bs, b.cin, res_in, res_in, generator=g)
    emb = torch.randn(bs, R.CIFAR10.emb_channels, generator=g)
    return x, emb


def test_layout_has_the_8x8_shapes():
    got = {(b.cin, b.skip_from or 0, b.attn, b.down) for _, b in blocks_8x8()}
    # Cin 256 (encoder, decoder in0 / in1), Cin 512 as the 256 + 256 concat (decoder), the down block, the attention block
    assert {(256, 0, False, False), (512, 256, False, False), (256, 0, False, True), (256, 0, True, False)} <= got


@pytest.mark.parametrize("bs", [1, 3, 16])
def test_blocks_8x8_against_fp64(net, sd, bs):
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.inference_mode():
        for index, b in blocks_8x8():
            x, emb = inputs(b, bs, 100 + index)
            got = run_block(net, index, b, x, emb)
            want = R.unet_block(sd64, b, x.double(), emb.double()).float()
            assert torch.isfinite(got).all(), b.key
            err = (got - want).abs().max().item()
            rel = ((got - want).norm() / want.norm()).item()
            assert err <= MAX_ABS and rel <= REL, f"{b.key} B={bs}: max_abs={err:.3e} rel_l2={rel:.3e}"


def test_blocks_8x8_batch_independent_at_512(net):
    """Every image of a B = 512 launch (256 image pairs, one per CU) equals the same image run in a batch of 16 or 5 (a half-empty
    last pair), bit for bit."""
    with torch.inference_mode():
        for index, b in blocks_8x8():
            x, emb = inputs(b, 512, 200 + index)
            big = run_block(net, index, b, x, emb)
            for lo, n in ((0, 16), (496, 16), (101, 5)):
                small = run_block(net, index, b, x[lo:lo + n].contiguous(), emb[lo:lo + n].contiguous())
                assert torch.equal(big[lo:lo + n], small), f"{b.key}: rows {lo}..{lo + n - 1} depend on the batch"


def test_blocks_8x8_generic_kernel():
    """The same fp64 checks with FASTGEN_AMD_CONV_WS=0 (read once per process, so in a child process)."""
    if os.environ.get("FASTGEN_AMD_CONV_WS") == "0":
        pytest.skip("already running with the generic kernel")
    env = dict(os.environ, FASTGEN_AMD_CONV_WS="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "against_fp64"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
