"""Record the EDM2 fixtures under tests/golden/ from the reference itself (read through oracle/_ref_import.py, CPU, fp32).

    python scripts/gen_golden_edm2.py                  every fixture
    python scripts/gen_golden_edm2.py drop_precond     only edm2_narrow_drop_precond_b2.pt (the others stay as they are)

Writes
  edm2_in64_s_state_dict_keys.txt  "name shape" per state_dict() entry of EDM2Precond(**EDM2_IN64_S_Config) (203 lines)
  edm2_narrow_b2.pt                tests/edm2_ref.py NARROW config, weights random_state_dict(seed 1234) (random gains), inputs from
                                   seeds: forward output (x0, no labels, eps + logvar), the embedding, every block output (subsampled),
                                   generator_fn (1 / 2 / 4 steps 'sde' with injected noise, 2 steps 'ode', a custom 2-step t_list) and
                                   one 4-step sample() with classifier-free guidance
  edm2_in64_s_b2.pt                the full EDM2-S network at B = 2, weights random_state_dict(seed 4321): forward output
  edm2_narrow_drop_precond_b2.pt   NARROW, the same weights and inputs, EDM2Precond(drop_precond = 'input' / 'output' / 'both'): the
                                   forward output of each, subsampled
Weights are not stored: tests/edm2_ref.py regenerates them from the seed."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle._ref_import import import_reference  # noqa: E402

import edm2_ref as D  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def sub(v):
    return D.subsample(v.detach(), 61)


def ref_net(mod, cfg, sd):
    net = mod.EDM2Precond(**cfg.kwargs())
    assert list(net.state_dict()) == list(sd)
    net.load_state_dict(sd, strict=True)
    return net.eval()


def inputs(cfg, B, seed):
    R = cfg.img_resolution
    t = torch.tensor([0.7, 12.0][:B], dtype=torch.float64)
    x = seeded((B, cfg.img_channels, R, R), seed) * t.reshape(-1, 1, 1, 1).float()
    cond = torch.nn.functional.one_hot(torch.arange(B) * 3 % cfg.label_dim, cfg.label_dim).float()
    return x, t, cond


def record_drop_precond(mod):
    cfg = D.NARROW
    sd = D.random_state_dict(cfg, seed=1234)
    x, t, cond = inputs(cfg, 2, 11)
    fx = {"t": t, "cond": cond}
    for drop in ("input", "output", "both"):
        net = mod.EDM2Precond(**cfg.kwargs(), drop_precond=drop)
        net.load_state_dict(sd, strict=True)
        with torch.inference_mode():
            fx[drop] = sub(net.eval()(x, t, condition=cond))
    torch.save(fx, os.path.join(OUT, "edm2_narrow_drop_precond_b2.pt"))


def main():
    _, _, model = import_reference()
    mod = importlib.import_module("fastgen.networks.EDM2.network")
    record_drop_precond(mod)
    if sys.argv[1:] == ["drop_precond"]:
        print("wrote", os.path.join(OUT, "edm2_narrow_drop_precond_b2.pt"))
        return
    torch.manual_seed(0)
    with torch.no_grad():
        full = mod.EDM2Precond(**D.IN64_S.kwargs())
    with open(os.path.join(OUT, "edm2_in64_s_state_dict_keys.txt"), "w") as f:
        for k, v in full.state_dict().items():
            f.write(f"{k} {','.join(str(s) for s in v.shape)}\n")
    del full

    cfg = D.NARROW
    sd = D.random_state_dict(cfg, seed=1234)
    net = ref_net(mod, cfg, sd)
    x, t, cond = inputs(cfg, 2, 11)
    trace, hooks = {}, []
    for group in ("enc", "dec"):
        for key, blk in getattr(net.unet, group).items():
            if isinstance(blk, mod.Block):
                hooks.append(blk.register_forward_hook(lambda m, a, o, k=f"unet.{group}.{key}": trace.__setitem__(k, o.detach().clone())))
    with torch.inference_mode():
        out = net(x, t, condition=cond).clone()
        out_nolabel = net(x, t, condition=None).clone()
        out_eps, logvar = net(x, t, condition=cond, fwd_pred_type="eps", return_logvar=True)
    for h in hooks:
        h.remove()
    with torch.no_grad():
        emb = D.embedding(sd, cfg, (t.log() / 4).float(), cond)
    fx = {"t": t, "cond": cond, "out": out, "out_nolabel": sub(out_nolabel), "out_eps": sub(out_eps), "logvar": logvar.clone(),
          "emb": emb, "blocks": {k: sub(v) for k, v in trace.items()}}
    noise = seeded((2, 3, 64, 64), 21)
    eps_all = [seeded((2, 3, 64, 64), s) for s in (22, 23, 24)]
    gen = {}
    with torch.inference_mode():
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
        neg = torch.nn.functional.one_hot(torch.tensor([5, 7]), cfg.label_dim).float()
        fx["sample_cfg"] = sub(net.sample(noise, condition=cond, neg_condition=neg, guidance_scale=2.0, num_steps=4))
    fx["gen"] = {k: (v if k in ("sde1", "sde4", "ode2") else sub(v)) for k, v in gen.items()}
    torch.save(fx, os.path.join(OUT, "edm2_narrow_b2.pt"))

    cfg = D.IN64_S
    sd = D.random_state_dict(cfg, seed=4321)
    net = ref_net(mod, cfg, sd)
    x, t, cond = inputs(cfg, 2, 12)
    with torch.inference_mode():
        out = net(x, t, condition=cond).clone()
    torch.save({"t": t, "cond_index": cond.argmax(1), "out": out}, os.path.join(OUT, "edm2_in64_s_b2.pt"))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
