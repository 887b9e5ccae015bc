"""The row-sweep consumer loop of the split-bf16 wave-specialised 3x3 kernel (conv_ws3.hip): per column shift every halo row is read
once and feeds the three tap rows, and the all-zero halo rows of tiles at the top / bottom image edge are skipped.  UNetBlocks of
the EDM CIFAR-10 U-Net against the fp64 CPU restatement at the bf16x3 parity tolerance (tests/test_gpu_parity.py), with the error
asserted separately on the output rows and columns next to a tile edge, so that a wrongly skipped or shifted row fails in a named
place; batch independence, bit for bit, at batches where workgroups take a second tile (the weight ring wraps into the next tile's
first step); and the same fp64 checks through the generic kernel (FASTGEN_AMD_CONV_WS=0)."""
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

# key -> what it reaches
CASES = {
    "model.enc.32x32_block0": "cin 128: four steps per tile, the ring's minimum",
    "model.enc.32x32_block1": "cin 256",
    "model.dec.32x32_block4": "256 + 128 concat: a step crosses from src1 to src2",
    "model.dec.32x32_block0": "256 + 256 concat",
    "model.dec.16x16_block0": "16x16: every tile is at the top or the bottom edge",
    "model.enc.8x8_block0": "8x8: every tile is at both edges, two images per tile",
    "model.dec.32x32_up": "16 -> 32 up block: conv1 reads the shifted residual",
}
BATCHES = {k: (1, 2, 3) if "8x8" in k else (1, 3) for k in CASES}  # 8x8: a full pair, and a last pair that is half empty


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return R.random_state_dict(R.CIFAR10, seed=1234)


@pytest.fixture(scope="module")
def sd64(sd):
    return {k: v.double() for k, v in sd.items()}


@pytest.fixture(scope="module")
def net(sd):
    n = EDMPrecond(compute_dtype="bf16x3", **KW)
    n.load_state_dict(sd, strict=True)
    return n.to(dev()).eval()


def block(key):
    enc, dec = R.layout(R.CIFAR10)
    blocks = [b for b in enc + dec if b.kind == "block"]
    (hit,) = [(i, b) for i, b in enumerate(blocks) if b.key == key]
    return hit


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
    res_in = b.res * 2 if b.down else b.res // 2 if b.up else b.res
    x = torch.randn(bs, b.cin, res_in, res_in, generator=g)
    emb = torch.randn(bs, R.CIFAR10.emb_channels, generator=g)
    return x, emb


def edge_lines(res, tile):
    """Rows (tile = 8) or columns (tile = 16) on either side of every tile edge, and the image's first and last."""
    return sorted({0, res - 1} | {t for k in range(tile, res, tile) for t in (k - 1, k)})


@pytest.mark.parametrize("key", list(CASES))
def test_block_against_fp64(net, sd64, key):
    index, b = block(key)
    with torch.inference_mode():
        for bs in BATCHES[key]:
            x, emb = inputs(b, bs, 300 + index)
            got = run_block(net, index, b, x, emb)
            want = R.unet_block(sd64, b, x.double(), emb.double()).float()
            assert got.shape == want.shape and torch.isfinite(got).all(), (key, bs)
            diff = (got - want).abs()
            for r in edge_lines(b.res, 8):
                err = diff[:, :, r, :].max().item()
                assert err <= MAX_ABS, f"{key} B={bs} output row {r}: max_abs={err:.3e}"
            for c in edge_lines(b.res, 16):
                err = diff[:, :, :, c].max().item()
                assert err <= MAX_ABS, f"{key} B={bs} output column {c}: max_abs={err:.3e}"
            err = diff.max().item()
            rel = ((got - want).norm() / want.norm()).item()
            assert err <= MAX_ABS and rel <= REL, f"{key} B={bs}: max_abs={err:.3e} rel_l2={rel:.3e}"


@pytest.mark.parametrize("key,big_bs", [("model.enc.32x32_block0", 33), ("model.enc.8x8_block0", 515)])
def test_second_tile_is_batch_independent(net, key, big_bs):
    """More tiles than the 256 CUs (33 x 8 = 264 at 32x32, 258 image pairs at 8x8): some workgroups take a second tile, whose first
    step's weights come through the ring refills of the previous tile's last step.  The first three images equal a B = 3 run bit for
    bit, and so do the last three, which are the ones the second tiles hold (the last 8x8 pair is half empty in both runs)."""
    index, b = block(key)
    with torch.inference_mode():
        x, emb = inputs(b, big_bs, 400 + index)
        big = run_block(net, index, b, x, emb)
        assert torch.isfinite(big).all()
        for lo in (0, big_bs - 3):
            small = run_block(net, index, b, x[lo:lo + 3].contiguous(), emb[lo:lo + 3].contiguous())
            assert torch.equal(big[lo:lo + 3], small), f"{key}: images {lo}..{lo + 2} of B={big_bs} differ from their B=3 run"


def test_generic_kernel_passes_the_same_references():
    """The same fp64 checks with FASTGEN_AMD_CONV_WS=0 (read once per process, so in a child process)."""
    if os.environ.get("FASTGEN_AMD_CONV_WS") == "0":
        pytest.skip("already running with the generic kernel")
    env = dict(os.environ, FASTGEN_AMD_CONV_WS="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "against_fp64"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
