"""DiT on a 32 x 32 token grid (input_size 64, patch 2: the 512 x 512 models), the parts that need no GPU: the drop-in module's state
dict at 1024 tokens, what fg_dit_create accepts and refuses, the workspace plan, and the fixture tests/golden/dit_in64_b2.pt
(scripts/gen_golden_dit_tokens.py: the reference's own DiT class on the restated timm stand-ins - the caveat of tests/test_dit.py,
carried over) pinned against the fp64 oracle."""
import ctypes
import dataclasses
import os

import pytest
import torch

from fastgen_amd import _lib
from oracle import dit_ref as R

S = dict(hidden_size=384, depth=12, num_heads=6)
CFGS = {"s64": dataclasses.replace(R.S_2, input_size=64), "xl64": dataclasses.replace(R.XL_2, input_size=64, depth=4)}
FG_EINVAL = 1


def inputs(cfg, B=2):
    x = torch.randn((B, cfg.in_channels, cfg.input_size, cfg.input_size), generator=torch.Generator().manual_seed(501))
    cond = torch.zeros(B, cfg.num_classes)
    cond[0, 417] = 1.0  # row 1 all-zero: the unconditional class
    return x, cond


def _config(input_size, dtype, hidden=384, heads=6, depth=2, patch=2):
    c = _lib.fg_dit_config()
    c.input_size, c.patch_size, c.in_channels, c.hidden_size, c.depth, c.num_heads = input_size, patch, 4, hidden, depth, heads
    c.mlp_hidden, c.embedding_rows, c.r_timestep, c.compute_dtype = 4 * hidden, 1001, 0, dtype
    return c


def _create(cfg):
    h = ctypes.c_void_p()
    rc = _lib.lib().fg_dit_create(ctypes.byref(cfg), ctypes.byref(h))
    return rc, h


def test_module_at_1024_tokens():
    from fastgen_amd.networks.DiT.network import DiT

    net = DiT(input_size=64, **S)
    sd = net.state_dict()
    assert tuple(sd["pos_embed"].shape) == (1, 1024, 384)
    assert torch.allclose(sd["pos_embed"], R.pos_embed_2d(384, 32).unsqueeze(0), atol=1e-6)
    res = net.load_state_dict(R.random_state_dict(CFGS["s64"]), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # every other entry has the shape it has at 256 tokens
    small = DiT(**S).state_dict()
    assert list(small) == list(sd)
    assert all(small[k].shape == sd[k].shape for k in sd if k != "pos_embed")


@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "fp8", None])
def test_module_modes_construct_at_1024_tokens(mode):
    from fastgen_amd.networks.DiT.network import DiT

    assert DiT(input_size=64, compute_dtype=mode, **S)._tokens == 1024


def test_module_refuses_exact_fp32_at_1024_tokens():
    from fastgen_amd.networks.DiT.network import DiT

    with pytest.raises(NotImplementedError, match="16 x 16"):
        DiT(input_size=64, compute_dtype="fp32", **S)
    assert DiT(input_size=32, compute_dtype="fp32", **S)._tokens == 256


@pytest.mark.parametrize("input_size,dtype", [(48, _lib.FG_DTYPE_BF16X3), (16, _lib.FG_DTYPE_BF16X3), (48, _lib.FG_DTYPE_BF16), (16, _lib.FG_DTYPE_F32),
                                              (64, _lib.FG_DTYPE_F32), (66, _lib.FG_DTYPE_BF16)])
def test_create_refuses(input_size, dtype):
    """grid 24, grid 8, exact fp32 at grid 32, and an input_size that the patch does not divide (patch 4 below)."""
    cfg = _config(input_size, dtype, patch=4 if input_size == 66 else 2)
    rc, h = _create(cfg)
    assert rc == FG_EINVAL and not h.value
    msg = _lib.lib().fg_last_error().decode()
    if input_size == 64:
        assert "fp32" in msg and "32 x 32" in msg
    else:
        assert "16 (256 tokens) or 32 (1024 tokens)" in msg


@pytest.mark.parametrize("input_size,dtype", [(32, _lib.FG_DTYPE_F32), (32, _lib.FG_DTYPE_BF16), (32, _lib.FG_DTYPE_BF16X3), (32, _lib.FG_DTYPE_FP8),
                                              (64, _lib.FG_DTYPE_BF16), (64, _lib.FG_DTYPE_BF16X3), (64, _lib.FG_DTYPE_FP8)])
def test_create_accepts(input_size, dtype):
    L = _lib.lib()
    rc, h = _create(_config(input_size, dtype))
    assert rc == 0, L.fg_last_error().decode()
    try:
        name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 4)()
        assert L.fg_dit_param_info(h, 0, ctypes.byref(name), ctypes.byref(ndim), shape) == 0
        assert name.value == b"pos_embed" and tuple(shape[:3]) == (1, (input_size // 2) ** 2, 384)
    finally:
        L.fg_dit_destroy(h)


@pytest.mark.parametrize("dtype", [_lib.FG_DTYPE_BF16, _lib.FG_DTYPE_BF16X3, _lib.FG_DTYPE_FP8])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_workspace_scales_with_the_tokens(dtype, B):
    """Every token tensor of the plan (dit_plan) is four times as large at 1024 tokens.  The vectors per image are not - Fourier
    features 256, five vectors of D, the modulation 6 D and 2 D, fp32: (256 + 13 D) * 4 bytes per image, each buffer rounded up to 256
    bytes - so the 1024-token plan is at least 4 x the 256-token plan less three times that part, and never below the 256-token plan
    of four times the batch less the same."""
    L = _lib.lib()
    D = 384
    per_image = B * 4 * (256 + 13 * D) + 32 * 256
    sizes = {}
    for input_size in (32, 64):
        rc, h = _create(_config(input_size, dtype))
        assert rc == 0
        sizes[input_size] = L.fg_dit_workspace_bytes(h, B)
        L.fg_dit_destroy(h)
    assert sizes[64] >= 4 * sizes[32] - 3 * per_image
    assert sizes[64] >= 3.9 * sizes[32]
    assert sizes[64] <= 4 * sizes[32]


@pytest.mark.parametrize("tag", ["s64", "xl64"])
def test_fixture_against_the_oracle(golden_dir, tag):
    """Relative L2 of the fp64 oracle against the recorded fp32 reference output <= 2e-5 (measured 3.2e-6 for s64, 2.7e-6 for xl64)."""
    fx = torch.load(os.path.join(golden_dir, "dit_in64_b2.pt"), weights_only=True)
    cfg = CFGS[tag]
    sd = {k: v.double() for k, v in R.random_state_dict(cfg, seed=77).items()}
    x, cond = inputs(cfg)
    tr = {}
    out = R.dit_forward(sd, cfg, x.double(), fx[f"{tag}/t"], cond.double(), trace=tr)
    want = fx[f"{tag}/out"].double()
    assert tuple(want.shape) == (2, 4, 64, 64)
    rel = float((out - want).norm() / want.norm())
    print(f"{tag}: oracle vs fixture rel L2 {rel:.2e}")
    assert rel <= 2e-5
    assert float((tr["c"] - fx[f"{tag}/c"].double()).abs().max()) < 1e-5
