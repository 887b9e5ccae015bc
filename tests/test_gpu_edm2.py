"""GPU parity of EDM2Precond against the reference-recorded fixtures and the functional restatement (tests/edm2_ref.py): forward,
every Block through fg_edm2_run_block, the fused few-step sampler (graph replay and eager), ragged batches, sample(), the full EDM2-S."""
import ctypes
import os

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.methods.model import FastGenModel
from fastgen_amd.networks.EDM2.network import EDM2Precond

import edm2_ref as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = {"bf16x3": dict(max_abs=5e-5, rel=2e-5), "bf16": dict(max_abs=5e-2, rel=1e-2)}  # as tests/test_gpu_dhariwal.py
MODES = ["bf16x3", "bf16"]


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def check(got, want, mode, what="", scale=1.0):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - want).abs().max().item()
    rel = ((got - want).norm() / want.norm().clamp_min(1e-12)).item()
    assert err <= TOL[mode]["max_abs"] * scale and rel <= TOL[mode]["rel"], f"{what}: max_abs={err:.3e} rel_l2={rel:.3e} ({mode})"


def make_net(cfg, sd, **kw):
    net = EDM2Precond(**cfg.kwargs(), **kw)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval().requires_grad_(False)


@pytest.fixture(scope="module")
def narrow():
    fx = torch.load(os.path.join(GOLDEN, "edm2_narrow_b2.pt"))
    sd = D.random_state_dict(D.NARROW, seed=1234)
    return fx, sd, make_net(D.NARROW, sd)


@pytest.mark.parametrize("mode", MODES)
def test_forward_narrow(narrow, mode):
    fx, sd, net = narrow
    net.compute_dtype = mode
    x = (seeded((2, 3, 64, 64), 11) * fx["t"].reshape(-1, 1, 1, 1).float()).cuda()
    t, cond = fx["t"].cuda(), fx["cond"].cuda()
    check(net(x, t, condition=cond), fx["out"], mode, "x0")
    check(D.subsample(net(x, t, condition=None).cpu()), fx["out_nolabel"], mode, "no labels")
    out, logvar = net(x, t, condition=cond, fwd_pred_type="eps", return_logvar=True)
    check(D.subsample(out.cpu()), fx["out_eps"], mode, "eps")
    assert (logvar.cpu() - fx["logvar"]).abs().max().item() <= 1e-5
    # sigma_shift applies in eval mode only
    shifted = make_net(D.NARROW, sd, sigma_shift=0.05, compute_dtype=mode)
    with torch.no_grad():
        want = D.precond_forward(sd, D.NARROW, x.cpu(), fx["t"], fx["cond"], sigma_shift=0.05)
        check(shifted(x, t, condition=cond), want, mode, "sigma_shift eval")
        shifted.train()
        check(shifted(x, t, condition=cond), fx["out"], mode, "sigma_shift train")


@pytest.mark.parametrize("mode", MODES)
def test_unconditional_small(mode):
    cfg = D.SMALL_UNCOND
    sd = D.random_state_dict(cfg, seed=77)
    net = make_net(cfg, sd, compute_dtype=mode)
    x = seeded((3, 3, 16, 16), 5) * 3.0
    t = torch.tensor([0.01, 1.0, 60.0], dtype=torch.float64)
    with torch.no_grad():
        want = D.precond_forward(sd, cfg, x, t, None)
    check(net(x.cuda(), t.cuda()), want, mode, "label_dim=0")


def _run_block(net, index, x1, x2, emb):
    dev = torch.device("cuda")
    dt, h = net._engine(dev)
    L = _lib.lib()
    B = x1.shape[0]
    key, cin, cout, rin, rout, attn = ctypes.c_char_p(), *(ctypes.c_int() for _ in range(5))
    _lib.check(L.fg_edm2_block_info(h, index, ctypes.byref(key), ctypes.byref(cin), ctypes.byref(cout), ctypes.byref(rin),
                                    ctypes.byref(rout), ctypes.byref(attn)))
    nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous().cuda()  # noqa: E731
    a1, a2, e = nhwc(x1), (nhwc(x2) if x2 is not None else None), emb.contiguous().cuda()
    out = torch.empty(B, rout.value, rout.value, cout.value, device=dev)
    ws = net._workspace(dt, h, B, dev)
    _lib.check(L.fg_edm2_run_block(h, index, ctypes.c_void_p(a1.data_ptr()), a1.shape[-1],
                                   ctypes.c_void_p(a2.data_ptr() if a2 is not None else None), a2.shape[-1] if a2 is not None else 0,
                                   ctypes.c_void_p(e.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, ctypes.c_void_p(ws.data_ptr()),
                                   ws.numel(), net._stream(dev)))
    return out.permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("mode", MODES)
def test_every_block(narrow, mode):
    _, sd, net = narrow
    net.compute_dtype = mode
    enc, dec, _, _, _ = D.layout(D.NARROW)
    B = 2
    with torch.no_grad():
        emb = D.embedding(sd, D.NARROW, torch.tensor([-0.5, 0.8]), torch.nn.functional.one_hot(torch.tensor([1, 4]), 10).float())
    for i, b in enumerate(enc + dec):
        c1 = b.cin - b.skip_c
        x1 = seeded((B, c1, b.res_in, b.res_in), 1000 + i)
        x2 = seeded((B, b.skip_c, b.res_in, b.res_in), 2000 + i) if b.skip_c else None
        with torch.no_grad():
            want = D.block(sd, b, D.NARROW, D.mp_cat(x1, x2, D.NARROW.concat_balance) if x2 is not None else x1, emb)
        check(_run_block(net, i, x1, x2, emb), want, mode, b.key)
    # clip_act active: a decoder block whose residual carries the scaled input past +-256
    i = len(enc) + 1
    b = dec[1]
    x1 = seeded((B, b.cin, b.res_in, b.res_in), 3000) * 1000.0
    with torch.no_grad():
        want = D.block(sd, b, D.NARROW, x1, emb)
    assert (want.abs() == 256).float().mean() > 0.1, "clip not active"
    check(_run_block(net, i, x1, None, emb), want, mode, b.key + " clipped", scale=256.0)


@pytest.mark.parametrize("mode", MODES)
def test_generator_fn_narrow(narrow, mode):
    fx, _, net = narrow
    net.compute_dtype = mode
    noise = seeded((2, 3, 64, 64), 21).cuda()
    eps = torch.stack([seeded((2, 3, 64, 64), s) for s in (22, 23, 24)]).cuda()
    cond = fx["cond"].cuda()
    for steps in (1, 2, 4):
        got = FastGenModel.generator_fn(net, noise, student_sample_steps=steps, condition=cond, student_sample_type="sde",
                                        eps=eps[: steps - 1])
        want = fx["gen"][f"sde{steps}"]
        check(got if steps != 2 else D.subsample(got.cpu()), want, mode, f"sde{steps}")
    got = FastGenModel.generator_fn(net, noise, student_sample_steps=2, condition=cond, student_sample_type="ode")
    check(got, fx["gen"]["ode2"], mode, "ode2")
    got = FastGenModel.generator_fn(net, noise, student_sample_steps=2, t_list=[80.0, 1.5, 0.0], condition=cond,
                                    student_sample_type="ode")
    check(D.subsample(got.cpu()), fx["gen"]["tlist2"], mode, "t_list")


@pytest.mark.parametrize("mode", MODES)
def test_graph_replay_bit_equal_to_eager(narrow, mode):
    _, sd, net = narrow
    net.compute_dtype = mode
    noise = seeded((3, 3, 64, 64), 31).cuda()
    cond = torch.nn.functional.one_hot(torch.arange(3), 10).float().cuda()
    tl = net.noise_scheduler.get_t_list(4, device="cpu")
    eager = net.few_step_sample(noise, cond, tl, sample_type="sde", seed=7, use_graph=False).clone()
    g1 = net.few_step_sample(noise, cond, tl, sample_type="sde", seed=7, use_graph=True).clone()
    captures, launches = _lib.graph_stats()
    g2 = net.few_step_sample(noise, cond, tl, sample_type="sde", seed=7, use_graph=True).clone()
    assert _lib.graph_stats() == (captures, launches + 1)
    assert torch.equal(eager, g1) and torch.equal(g1, g2)
    # the same graph replayed with a new t_list (same zero pattern) and seed equals an eager run with those
    tl2 = torch.tensor([60.0, 9.0, 2.0, 0.3, 0.0], dtype=torch.float64)
    g3 = net.few_step_sample(noise, cond, tl2, sample_type="sde", seed=11, use_graph=True).clone()
    assert _lib.graph_stats() == (captures, launches + 2)
    e3 = net.few_step_sample(noise, cond, tl2, sample_type="sde", seed=11, use_graph=False).clone()
    assert torch.equal(g3, e3) and not torch.equal(g3, g1)
    # the per-step loop through forward() and the noise schedule, with the same injected noise
    eps = torch.randn(3, 3, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    fused = net.few_step_sample(noise, cond, tl, sample_type="sde", eps=eps, use_graph=True)
    ns = net.noise_scheduler
    x = ns.latents(noise=noise, t_init=tl[0].cuda())
    for i in range(4):
        x0 = net(x, tl[i].cuda().expand(3), condition=cond)
        if tl[i + 1] > 0:
            x = ns.forward_process(x0, eps[i], tl[i + 1].cuda().expand(3))
    assert (fused - x0).abs().max().item() <= 1e-4 * x0.abs().max().item()
    # sigma_shift (eval mode only) is baked into the captured graph: with every buffer the same, so that the graph key matches, a
    # train() / eval() flip must still not replay the graph captured in the other mode
    shifted = make_net(D.NARROW, sd, sigma_shift=0.05, compute_dtype=mode)
    out = torch.empty_like(noise)
    runs = []
    with torch.no_grad():
        for training in (False, True, False):
            shifted.train(training)
            g = shifted.few_step_sample(noise, cond, tl, sample_type="sde", seed=7, use_graph=True, out=out).clone()
            e = shifted.few_step_sample(noise, cond, tl, sample_type="sde", seed=7, use_graph=False)
            assert torch.equal(g, e), f"training={training}"
            runs.append(g)
    assert not torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


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


@pytest.mark.parametrize("mode", MODES)
def test_sample_cfg(narrow, mode):
    fx, _, net = narrow
    net.compute_dtype = mode
    noise = seeded((2, 3, 64, 64), 21).cuda()
    cond = fx["cond"].cuda()
    neg = torch.nn.functional.one_hot(torch.tensor([5, 7]), 10).float().cuda()
    with torch.no_grad():
        got = net.sample(noise, condition=cond, neg_condition=neg, guidance_scale=2.0, num_steps=4)
        check(D.subsample(got.cpu()), fx["sample_cfg"], mode, "sample cfg")
        # the per-step loop written out
        ns = net.noise_scheduler
        sig = ns.get_t_list(4, device=noise.device)
        x = ns.latents(noise=noise, t_init=sig[0])
        for s, s_next in zip(sig[:-1], sig[1:]):
            tb = s.expand(2)
            x0 = net(torch.cat([x, x]), torch.cat([tb, tb]), condition=torch.cat([neg, cond]))
            u, c = x0.chunk(2)
            x0 = u + 2.0 * (c - u)
            d = (x - x0) / tb.reshape(-1, 1, 1, 1)
            x = x + (s_next - s).to(x.dtype) * d
        assert torch.equal(got, x)


@pytest.mark.parametrize("mode,tol", [("bf16x3", 1e-4), ("bf16", 2e-2)])
def test_full_in64_s(mode, tol):
    fx = torch.load(os.path.join(GOLDEN, "edm2_in64_s_b2.pt"))
    net = make_net(D.IN64_S, D.random_state_dict(D.IN64_S, seed=4321), compute_dtype=mode)
    x = (seeded((2, 3, 64, 64), 12) * fx["t"].reshape(-1, 1, 1, 1).float()).cuda()
    cond = torch.nn.functional.one_hot(fx["cond_index"], 1000).float().cuda()
    out = net(x, fx["t"].cuda(), condition=cond).cpu()
    rel = ((out - fx["out"]).norm() / fx["out"].norm()).item()
    assert torch.isfinite(out).all() and rel <= tol, rel
    noise = seeded((2, 3, 64, 64), 13).cuda()
    for steps in (1, 4):
        img = FastGenModel.generator_fn(net, noise, student_sample_steps=steps, condition=cond, student_sample_type="sde", seed=3)
        assert img.shape == noise.shape and torch.isfinite(img).all()
