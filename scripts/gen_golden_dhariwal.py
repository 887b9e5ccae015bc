"""Record the DhariwalUNet fixtures under tests/golden/ from the reference itself (read through oracle/_ref_import.py, CPU, fp32).

    python scripts/gen_golden_dhariwal.py

Writes
  dhariwal_in64_state_dict_keys.txt  "name shape" per state_dict() entry of EDMPrecond(**EDM_ImageNet64_Config) (555 lines)
  dhariwal_narrow_b2.pt              fixture (a): tests/dhariwal_ref.py NARROW config, weights random_state_dict(seed 1234), inputs from seeds:
                                     forward output, emb, every block output (subsampled), generator_fn (1 / 2 / 4 steps 'sde' with injected
                                     noise, 2 steps 'ode', a custom 2-step t_list)
  dhariwal_in64_b2.pt                fixture (b): the full in64 config at B = 2, weights random_state_dict(seed 4321): forward output
Weights are not stored: tests/dhariwal_ref.py regenerates them from the seed."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle._ref_import import import_reference  # noqa: E402

import dhariwal_ref as D  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


SAMPLE = 61  # stride of the recorded subsamples (D.subsample)


def sub(v):
    return D.subsample(v.detach(), SAMPLE)


def ref_net(edm_net, cfg: D.DhariwalConfig, sd):
    net = edm_net.EDMPrecond(**cfg.kwargs())
    ref_sd = net.state_dict()
    assert list(ref_sd) == list(sd), set(ref_sd) ^ set(sd)
    for k in ref_sd:
        assert tuple(ref_sd[k].shape) == tuple(sd[k].shape), k
    net.load_state_dict(sd, strict=True)
    return net.eval()


def inputs(cfg: D.DhariwalConfig, B: int, seed: int):
    R = cfg.img_resolution
    t = torch.tensor([0.7, 12.0][:B], dtype=torch.float64)
    x = seeded((B, cfg.img_channels, R, R), seed) * t.reshape(-1, 1, 1, 1).float()
    cond = torch.nn.functional.one_hot(torch.arange(B) * 3 % cfg.label_dim, cfg.label_dim).float()
    return x, t, cond


def main():
    edm_net, _, model = import_reference()
    torch.manual_seed(0)
    with torch.no_grad():
        full = edm_net.EDMPrecond(**D.IN64.kwargs())
    with open(os.path.join(OUT, "dhariwal_in64_state_dict_keys.txt"), "w") as f:
        for k, v in full.state_dict().items():
            f.write(f"{k} {','.join(str(s) for s in v.shape)}\n")
    assert [k for k in full.state_dict()] == list(D.state_shapes(D.IN64)), "state_shapes disagrees with the reference"
    del full

    # (a) narrow net at full resolution
    cfg = D.NARROW
    sd = D.random_state_dict(cfg, seed=1234)
    net = ref_net(edm_net, cfg, sd)
    x, t, cond = inputs(cfg, 2, 11)
    trace, hooks = {}, []
    for group in ("enc", "dec"):
        for key, blk in getattr(net.model, group).items():
            if isinstance(blk, edm_net.UNetBlock):
                hooks.append(blk.register_forward_hook(lambda m, a, o, k=f"{group}.{key}": trace.__setitem__(k, o.detach().clone())))
    hooks.append(net.model.map_layer1.register_forward_hook(lambda m, a, o: trace.__setitem__("map_layer1", o.detach().clone())))
    with torch.inference_mode():
        out = net(x, t, condition=cond, fwd_pred_type="x0").clone()
        out_nolabel = net(x, t, condition=None, fwd_pred_type="x0").clone()
        out_eps, logvar = net(x, t, condition=cond, fwd_pred_type="eps", return_logvar=True)
    for h in hooks:
        h.remove()
    lab = torch.nn.functional.linear(cond, sd["model.map_label.weight"])
    # whole tensors where the tests compare them element by element, SAMPLE-strided subsamples elsewhere (keeps the file small);
    # inputs are regenerated from their seeds (x: 11, noise: 21, eps: 22 23 24)
    fx = {"t": t, "cond": cond, "out": out, "out_nolabel": sub(out_nolabel), "out_eps": sub(out_eps), "logvar": logvar.clone(),
          "emb": torch.nn.functional.silu(trace.pop("map_layer1") + lab), "blocks": {k: sub(v) for k, v in trace.items()},
          "x_check": sub(x)}
    noise = seeded((2, 3, 64, 64), 21)
    eps_all = [seeded((2, 3, 64, 64), s) for s in (22, 23, 24)]
    gen = {}
    for steps in (1, 2, 4):
        it = iter(eps_all)
        orig = torch.randn_like
        try:
            torch.randn_like = lambda a, **k: next(it).to(a.dtype)
            gen[f"sde{steps}"] = model.FastGenModel.generator_fn(net, noise, student_sample_steps=steps, condition=cond,
                                                                 student_sample_type="sde").clone()
        finally:
            torch.randn_like = orig
    gen["ode2"] = model.FastGenModel.generator_fn(net, noise, student_sample_steps=2, condition=cond, student_sample_type="ode").clone()
    gen["tlist2"] = model.FastGenModel.generator_fn(net, noise, student_sample_steps=2, t_list=[80.0, 1.5, 0.0], condition=cond,
                                                    student_sample_type="ode").clone()
    gen = {k: (v if k in ("sde1", "sde4", "ode2") else sub(v)) for k, v in gen.items()}
    fx.update({"gen": gen})
    torch.save(fx, os.path.join(OUT, "dhariwal_narrow_b2.pt"))

    # (b) the whole EDM_ImageNet64_Config network, forward only
    cfg = D.IN64
    sd = D.random_state_dict(cfg, seed=4321)
    net = ref_net(edm_net, cfg, sd)
    x, t, cond = inputs(cfg, 2, 12)
    with torch.inference_mode():
        out = net(x, t, condition=cond, fwd_pred_type="x0").clone()
    torch.save({"t": t, "cond_index": cond.argmax(1), "out": out}, os.path.join(OUT, "dhariwal_in64_b2.pt"))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
