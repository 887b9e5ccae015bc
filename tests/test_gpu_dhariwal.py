"""GPU parity of EDMPrecond(model_type="DhariwalUNet") against the reference-recorded fixtures and the functional restatement
(tests/dhariwal_ref.py): forward, the fused few-step sampler (graph replay and eager), ragged batches, the full in64 network."""
import os

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.methods.model import FastGenModel
from fastgen_amd.networks.EDM.network import EDMPrecond

import dhariwal_ref as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = {"bf16x3": dict(max_abs=5e-5, rel=2e-5), "bf16": dict(max_abs=5e-2, rel=1e-2)}  # tests/test_gpu_parity.py


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def check(got, want, mode, what=""):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - want).abs().max().item()
    rel = ((got - want).norm() / want.norm().clamp_min(1e-12)).item()
    assert err <= TOL[mode]["max_abs"] and rel <= TOL[mode]["rel"], f"{what}: max_abs={err:.3e} rel_l2={rel:.3e} ({mode})"


@pytest.fixture(scope="module")
def narrow():
    fx = torch.load(os.path.join(GOLDEN, "dhariwal_narrow_b2.pt"))
    sd = D.random_state_dict(D.NARROW, seed=1234)
    net = EDMPrecond(**D.NARROW.kwargs())
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval().requires_grad_(False)
    return fx, sd, net


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_forward_narrow(narrow, mode):
    fx, _, net = narrow
    net.compute_dtype = mode
    x = (seeded((2, 3, 64, 64), 11) * fx["t"].reshape(-1, 1, 1, 1).float()).cuda()
    t, cond = fx["t"].cuda(), fx["cond"].cuda()
    check(net(x, t, condition=cond), fx["out"], mode, "x0")
    check(D.subsample(net(x, t, condition=None).cpu()), fx["out_nolabel"], mode, "no labels")
    out, logvar = net(x, t, condition=cond, fwd_pred_type="eps", return_logvar=True)
    check(D.subsample(out.cpu()), fx["out_eps"], mode, "eps")
    assert (logvar.cpu() - fx["logvar"]).abs().max().item() <= 1e-5


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_generator_fn_narrow(narrow, mode):
    fx, _, net = narrow
    net.compute_dtype = mode
    noise = seeded((2, 3, 64, 64), 21).cuda()
    eps = torch.stack([seeded((2, 3, 64, 64), s) for s in (22, 23, 24)]).cuda()
    cond = fx["cond"].cuda()
    for steps in (1, 4):
        got = FastGenModel.generator_fn(net, noise, student_sample_steps=steps, condition=cond, student_sample_type="sde",
                                        eps=eps[: steps - 1])
        check(got, fx["gen"][f"sde{steps}"], mode, f"sde{steps}")
    got = FastGenModel.generator_fn(net, noise, student_sample_steps=2, condition=cond, student_sample_type="ode")
    check(got, fx["gen"]["ode2"], mode, "ode2")
    got = FastGenModel.generator_fn(net, noise, student_sample_steps=2, t_list=[80.0, 1.5, 0.0], condition=cond,
                                    student_sample_type="ode")
    check(D.subsample(got.cpu()), fx["gen"]["tlist2"], mode, "t_list")


def test_ragged_batches(narrow):
    _, sd, net = narrow
    net.compute_dtype = "bf16x3"
    for B in (1, 3, 5):
        x = seeded((B, 3, 64, 64), 100 + B) * 2.0
        t = torch.linspace(0.05, 40.0, B, dtype=torch.float64)
        cond = torch.nn.functional.one_hot(torch.arange(B) % 10, 10).float()
        with torch.no_grad():
            want = D.precond_forward(sd, D.NARROW, x, t, cond)
        check(net(x.cuda(), t.cuda(), condition=cond.cuda()), want, "bf16x3", f"B={B}")


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_graph_replay_bit_equal_to_eager(narrow, mode):
    _, _, net = narrow
    net.compute_dtype = mode
    noise = seeded((3, 3, 64, 64), 31).cuda()
    cond = torch.nn.functional.one_hot(torch.arange(3), 10).float().cuda()
    tl = net.noise_scheduler.get_t_list(4, device="cpu")
    eager = net.few_step_sample(noise, cond, tl, sample_type="sde", seed=7, use_graph=False).clone()
    g1 = net.few_step_sample(noise, cond, tl, sample_type="sde", seed=7, use_graph=True).clone()
    captures, launches = _lib.graph_stats()
    g2 = net.few_step_sample(noise, cond, tl, sample_type="sde", seed=7, use_graph=True).clone()
    assert _lib.graph_stats() == (captures, launches + 1)  # a replay
    assert torch.equal(eager, g1) and torch.equal(g1, g2)
    # the per-step loop through forward() and the noise schedule, with the same device noise
    eps = torch.randn(3, 3, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    fused = net.few_step_sample(noise, cond, tl, sample_type="sde", eps=eps, use_graph=True)
    ns = net.noise_scheduler
    x = ns.latents(noise=noise, t_init=tl[0].cuda())
    for i in range(4):
        tb = tl[i].cuda().expand(3)
        x0 = net(x, tb, condition=cond)
        if tl[i + 1] > 0:
            x = ns.forward_process(x0, eps[i], tl[i + 1].cuda().expand(3))
    assert (fused - x0).abs().max().item() <= 1e-4 * x0.abs().max().item()


@pytest.mark.parametrize("mode,tol", [("bf16x3", 1e-4), ("bf16", 2e-2)])
def test_full_in64(mode, tol):
    fx = torch.load(os.path.join(GOLDEN, "dhariwal_in64_b2.pt"))
    net = EDMPrecond(**D.IN64.kwargs(), compute_dtype=mode)
    net.load_state_dict(D.random_state_dict(D.IN64, seed=4321), strict=True)
    net = net.cuda().eval().requires_grad_(False)
    x = (seeded((2, 3, 64, 64), 12) * fx["t"].reshape(-1, 1, 1, 1).float()).cuda()
    cond = torch.nn.functional.one_hot(fx["cond_index"], 1000).float().cuda()
    out = net(x, fx["t"].cuda(), condition=cond).cpu()
    rel = ((out - fx["out"]).norm() / fx["out"].norm()).item()
    assert torch.isfinite(out).all() and rel <= tol, rel
    # one graph-captured call samples 1 and 4 steps
    noise = seeded((2, 3, 64, 64), 13).cuda()
    for steps in (1, 4):
        img = FastGenModel.generator_fn(net, noise, student_sample_steps=steps, condition=cond, student_sample_type="sde", seed=3)
        assert img.shape == noise.shape and torch.isfinite(img).all()
    # the 4-step sampler equals the per-step loop through forward() and the noise schedule with the same explicit noise
    eps = torch.stack([seeded((2, 3, 64, 64), s) for s in (14, 15, 16)]).cuda()
    fused = FastGenModel.generator_fn(net, noise, student_sample_steps=4, condition=cond, student_sample_type="sde", eps=eps)
    ns = net.noise_scheduler
    tl = ns.get_t_list(4, device="cpu")
    x = ns.latents(noise=noise, t_init=tl[0].cuda())
    for i in range(4):
        x0 = net(x, tl[i].cuda().expand(2), condition=cond)
        if tl[i + 1] > 0:
            x = ns.forward_process(x0, eps[i], tl[i + 1].cuda().expand(2))
    assert (fused - x0).abs().max().item() <= 1e-4 * x0.abs().max().item()
