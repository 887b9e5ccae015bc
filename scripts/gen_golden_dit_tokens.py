"""Record the 1024-token DiT fixture under tests/golden/ from the reference's own `DiT` class (read through oracle/_ref_import.py on
the restated timm stand-ins of oracle/_timm_restated.py, CPU, fp32).

    python scripts/gen_golden_dit_tokens.py

Writes
  dit_in64_b2.pt   two tags at input_size 64 (latent 64, patch 2: a 32 x 32 token grid), B = 2:
                     s64    S width (384, 6 heads of 64), depth 12
                     xl64   XL width (1152, 16 heads of 72), depth 4
                   per tag the forward output, `t` and the conditioning vector c.
Weights are not stored: oracle.dit_ref.random_state_dict(cfg, seed=77) regenerates them.  Inputs as in oracle/gen_golden.py's
dit_fixture: x from seed 501, class 417 in row 0, row 1 all-zero (the unconditional class)."""
import dataclasses
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import _ref_import, _timm_restated, dit_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CONFIGS = {"s64": dataclasses.replace(dit_ref.S_2, input_size=64), "xl64": dataclasses.replace(dit_ref.XL_2, input_size=64, depth=4)}
SEED, B = 77, 2


def inputs(cfg):
    x = torch.randn((B, cfg.in_channels, cfg.input_size, cfg.input_size), generator=torch.Generator().manual_seed(501))
    t = torch.tensor([0.731, 0.094], dtype=torch.float64)
    cond = torch.zeros(B, cfg.num_classes)
    cond[0, 417] = 1.0
    return x, t, cond


def main():
    _ref_import.install_stubs()
    _timm_restated.install()
    if _ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, _ref_import.REFERENCE_ROOT)
    import fastgen.networks.DiT.network as dit_net

    fx = {}
    for tag, cfg in CONFIGS.items():
        sd = dit_ref.random_state_dict(cfg, seed=SEED)
        net = dit_net.DiT(input_size=cfg.input_size, patch_size=cfg.patch_size, in_channels=cfg.in_channels, hidden_size=cfg.hidden_size,
                          depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, class_dropout_prob=cfg.class_dropout_prob,
                          enable_class_dropout=False, num_classes=cfg.num_classes, learn_sigma=False, r_timestep=cfg.r_timestep,
                          scale_t=cfg.scale_t)
        assert list(net.state_dict().keys()) == list(sd.keys())
        net.load_state_dict(sd, strict=True)
        net.eval()
        x, t, cond = inputs(cfg)
        with torch.inference_mode():
            out = net(x, t, condition=cond)
        tr = {}
        oo = dit_ref.dit_forward({k: v.double() for k, v in sd.items()}, cfg, x.double(), t, cond.double(), trace=tr)
        rel = float((oo - out.double()).norm() / out.double().norm())
        print(f"{tag}: out {tuple(out.shape)}, oracle (fp64) vs reference (fp32) rel L2 {rel:.2e}")
        assert rel <= 2e-5, rel
        fx.update({f"{tag}/out": out.clone(), f"{tag}/t": t, f"{tag}/c": tr["c"].float().clone()})
    path = os.path.join(OUT, "dit_in64_b2.pt")
    torch.save(fx, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
