"""GPU parity tests (run with -m gpu on an MI355X).  Every check goes through the C ABI of libfastgen_amd.so and
compares with (a) golden vectors recorded from the reference and (b) the CPU oracle on the same seeded inputs.

Stated tolerances (north_star: "within a stated fp32 tolerance"):
  fp32 mode (v_mfma_f32_32x32x2_f32, exact fp32 arithmetic, different summation order than the CPU):
      per block  max|err| <= 5e-5 on O(1) activations;   whole forward / 4-step sampler  max|err| <= 5e-5
      (the reference's own cross-implementation bar is rel < 1e-3 and max < 1e-2, tests/test_fsdp.py:604)
  bf16x3 mode (fp32 tensors; convolutions as three bf16 MFMAs per product on hi/lo-split operands, ~2^-17 per product — the
      default arithmetic outside autocast): THE SAME fp32 tolerance as the exact mode, max|err| <= 5e-5 and relative L2 <= 2e-5
      (measured 1.1e-5 / 7.8e-6 on the whole forward; TF32, what the reference runs on its GPUs, is 2^-11 per product)
  bf16 mode (bf16 MFMA operands, fp32 accumulate / residual stream / norm statistics / softmax):
      relative L2 error <= 1e-2 and max|err| <= 5e-2
  sampler elementwise steps: bit-exact (fp64 arithmetic, one rounding).
"""
import ctypes
import os

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.methods.consistency_model.mean_flow import MeanFlowModel
from fastgen_amd.methods.model import FastGenModel
from fastgen_amd.networks.EDM.network import EDMPrecond
from oracle import edm_ref as R

pytestmark = pytest.mark.gpu

KW = dict(img_resolution=32, img_channels=3, label_dim=10, sigma_shift=0.0, sigma_data=0.5, model_type="SongUNet",
          augment_dim=9, model_channels=128, channel_mult=[2, 2, 2], channel_mult_noise=1, embedding_type="positional",
          encoder_type="standard", decoder_type="standard", resample_filter=[1, 1], dropout=0.0, label_dropout=0,
          r_timestep=False, drop_precond=None)
TOL = {"fp32": dict(max_abs=5e-5, rel=2e-5), "bf16x3": dict(max_abs=5e-5, rel=2e-5), "bf16": dict(max_abs=5e-2, rel=1e-2)}


def dev():
    return torch.device("cuda:0")


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def check(got, want, mode, what=""):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - want).abs().max().item()
    rel = ((got - want).norm() / want.norm().clamp_min(1e-12)).item()
    assert err <= TOL[mode]["max_abs"] and rel <= TOL[mode]["rel"], f"{what}: max_abs={err:.3e} rel_l2={rel:.3e} ({mode})"


@pytest.fixture(scope="module")
def sd():
    return R.random_state_dict(R.CIFAR10, seed=1234)


@pytest.fixture(scope="module")
def nets(sd):
    out = {}
    for mode in ("fp32", "bf16x3", "bf16"):
        n = EDMPrecond(compute_dtype=mode, **KW)
        n.load_state_dict(sd, strict=True)
        out[mode] = n.to(dev()).eval()
    return out


def load(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), weights_only=True)


# ---- op level -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c1,c2,hw", [(256, 0, 64), (128, 0, 1024), (256, 128, 1024), (256, 256, 256)])
def test_gn_coeffs(c1, c2, hw):
    """GroupNorm statistics + affine folding against torch.group_norm (EDM/network.py:141-149), incl. the virtual
    concat with 12 channels per group (C = 384)."""
    B, C = 3, c1 + c2
    x = seeded((B, hw, C), 1) * 1.7 + 0.3
    gamma, beta = 1 + 0.1 * seeded((C,), 2), 0.1 * seeded((C,), 3)
    x1, x2 = x[..., :c1].contiguous().to(dev()), x[..., c1:].contiguous().to(dev())
    gd, bd = gamma.to(dev()), beta.to(dev())  # keep the device copies alive across the call
    ab = torch.empty(B, C, 2, device=dev())
    _lib.check(_lib.lib().fg_op_gn_coeffs(x1.data_ptr(), c1, x2.data_ptr() if c2 else None, c2, gd.data_ptr(),
                                          bd.data_ptr(), 1e-6, ab.data_ptr(), B, hw, None))
    torch.cuda.synchronize()
    ab = ab.cpu()
    y = ab[..., 0][:, None, :] * x + ab[..., 1][:, None, :]
    want = torch.nn.functional.group_norm(x.permute(0, 2, 1).contiguous(), 32, gamma, beta, 1e-6).permute(0, 2, 1)
    assert (y - want).abs().max() < 2e-5


def test_sampler_elementwise_bit_exact():
    L = _lib.lib()
    x, e = seeded((4, 3, 32, 32), 11), seeded((4, 3, 32, 32), 12)
    xd, ed, od = x.to(dev()), e.to(dev()), torch.empty(4, 3, 32, 32, device=dev())
    for sched, sid, ts in (("edm", _lib.FG_SCHEDULE_EDM, (79.5638, 17.498123, 0.1726, 0.002)),
                           ("rf", _lib.FG_SCHEDULE_RF, (0.999, 0.7492, 0.2497, 1e-7))):
        for t in ts:
            tt = torch.tensor(t, dtype=torch.float64)
            _lib.check(L.fg_op_forward_process(xd.data_ptr(), ed.data_ptr(), t, sid, od.data_ptr(), x.numel(), None))
            assert torch.equal(od.cpu(), R.forward_process(x, e, tt.expand(4), sched))
            _lib.check(L.fg_op_latents(xd.data_ptr(), t, od.data_ptr(), x.numel(), None))
            assert torch.equal(od.cpu(), R.latents(x, tt))
            _lib.check(L.fg_op_x0_to_eps(xd.data_ptr(), ed.data_ptr(), t, sid, od.data_ptr(), x.numel(), None))
            assert torch.equal(od.cpu(), R.x0_to_eps(x, e, tt.expand(4), schedule=sched))


@pytest.mark.parametrize("shape", [(512, 3, 32, 32), (7, 3, 32, 32), (3, 1, 5, 9), (0, 3, 32, 32)])
def test_images_to_uint8_bit_exact(shape):
    """Sample-writer bytes (scripts/fid/compute_fid_from_ckpts.py:199) against the oracle: exact, including values on the
    truncation boundaries and saturating ones; B = 512 is the bench batch, the others are ragged / empty."""
    from fastgen_amd.utils.images import images_to_uint8

    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=g) * 0.7
    if x.numel():
        flat = x.view(-1)
        k = torch.arange(0, 256, dtype=torch.float32)
        edge = torch.cat([(k - 128) / 127.5, torch.nextafter((k - 128) / 127.5, torch.tensor(-9.0)), torch.tensor([-9.0, 9.0, -1.0, 1.0])])
        n = min(edge.numel(), flat.numel())
        flat[:n] = edge[:n]
    got = images_to_uint8(x.cuda())
    want = R.images_to_uint8(x)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)
    with pytest.raises(RuntimeError):
        images_to_uint8(x)  # CPU tensor: no fallback
    with pytest.raises(ValueError):
        images_to_uint8(torch.zeros(3, 4, device="cuda"))


def test_randn_device_generator():
    L = _lib.lib()
    n = 1 << 20
    a, b, c = (torch.empty(n, device=dev()) for _ in range(3))
    _lib.check(L.fg_op_randn(a.data_ptr(), n, 42, 0, None))
    _lib.check(L.fg_op_randn(b.data_ptr(), n, 42, 0, None))
    _lib.check(L.fg_op_randn(c.data_ptr(), n, 43, 0, None))
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert abs(a.mean().item()) < 5e-3 and abs(a.std().item() - 1) < 5e-3
    assert abs((a ** 4).mean().item() - 3.0) < 0.1 and a.abs().max() < 7  # normal kurtosis, sane tails
    assert abs(torch.corrcoef(torch.stack([a[:-1], a[1:]]))[0, 1].item()) < 5e-3
    odd = torch.empty(7, device=dev())  # ragged tail
    _lib.check(L.fg_op_randn(odd.data_ptr(), 7, 42, 0, None))
    assert torch.equal(odd, a[:7])


# ---- block level: the nine UNetBlock variants recorded from the reference ------------------------------------------


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_blocks_against_reference_golden(nets, golden_dir, mode):
    fx = load(golden_dir, "blocks_full.pt")
    net = nets[mode]
    L = _lib.lib()
    enc, dec = R.layout(R.CIFAR10)
    blocks = [b for b in enc + dec if b.kind == "block"]
    with torch.inference_mode():
        dt, h = net._engine(dev())
        assert L.fg_edm_num_blocks(h) == len(blocks) == 33
        names = sorted({k.split("/")[0] for k in fx if "/" in k})
        assert len(names) == 9
        for n in names:
            key = fx[f"{n}/key"]
            bi = [i for i, b in enumerate(blocks) if b.key == key][0]
            b = blocks[bi]
            kp, ci, co, ri, ro, at = (ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int())
            _lib.check(L.fg_edm_block_info(h, bi, ctypes.byref(kp), ctypes.byref(ci), ctypes.byref(co), ctypes.byref(ri),
                                           ctypes.byref(ro), ctypes.byref(at)))
            assert kp.value.decode() == key and ci.value == b.cin and co.value == b.cout and bool(at.value) == b.attn
            bs = fx[f"{n}/out"].shape[0]
            xb = seeded((bs, b.cin, ri.value, ri.value), int(fx[f"{n}/seed"]))
            c2 = b.skip_from or 0
            c1 = b.cin - c2
            x1 = nhwc(xb[:, :c1]).to(dev())
            x2 = nhwc(xb[:, c1:]).to(dev()) if c2 else None
            emb = fx["emb"][:bs].to(dev()).contiguous()
            out = torch.empty(bs, b.res, b.res, b.cout, device=dev())
            ws = net._workspace(dt, h, bs, dev())
            _lib.check(L.fg_edm_run_block(h, bi, x1.data_ptr(), c1, x2.data_ptr() if c2 else None, c2, emb.data_ptr(),
                                          out.data_ptr(), bs, ws.data_ptr(), ws.numel(), None))
            check(nchw(out), fx[f"{n}/out"], mode, f"block {n} {key}")


# ---- whole network -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_forward_against_reference_golden(nets, golden_dir, mode):
    fx = load(golden_dir, "forward_full_b2.pt")
    net = nets[mode]
    x = (seeded((2, 3, 32, 32), 21) * fx["t"].reshape(2, 1, 1, 1).float()).to(dev())
    with torch.inference_mode():
        out = net(x, fx["t"].to(dev()), condition=fx["cond"].to(dev()), fwd_pred_type="x0")
    check(out, fx["out"], mode, "EDMPrecond.forward B=2")
    assert out.dtype == torch.float32 and out.shape == (2, 3, 32, 32)


def test_forward_api_variants(nets, sd):
    net = nets["fp32"]
    B = 3
    x, t = seeded((B, 3, 32, 32), 5) * 3, torch.tensor([5.0, 0.5, 40.0], dtype=torch.float64)
    cond = torch.nn.functional.one_hot(torch.tensor([1, 2, 3]), 10).float()
    with torch.inference_mode():
        want = R.edm_precond_forward(sd, R.CIFAR10, x, t, cond)
        xd, td, cd = x.to(dev()), t.to(dev()), cond.to(dev())
        check(net(xd, td, condition=cd), want, "fp32", "default fwd_pred_type")
        # unconditional: the reference substitutes zeros([1, label_dim]) (EDM/network.py:919-925)
        check(net(xd, td, condition=None), R.edm_precond_forward(sd, R.CIFAR10, x, t, None), "fp32", "condition=None")
        # eps / flow prediction types go through noise_scheduler.convert_model_output
        eps = net(xd, td, condition=cd, fwd_pred_type="eps").cpu()
        assert torch.allclose(eps, R.x0_to_eps(x, want, t), atol=5e-4)
        flow = net(xd, td, condition=cd, fwd_pred_type="flow").cpu()
        assert torch.allclose(flow, eps, atol=1e-6)  # EDM: flow == eps-style quotient (x_t - x0)/t
        # float32 timesteps and a scalar t broadcast are accepted like the reference's t.expand(B)
        check(net(xd, td.float(), condition=cd), want, "bf16", "fp32 t")
        out, logvar = net(xd, td, condition=cd, return_logvar=True)
        assert logvar.shape == (B, 1)
        c_noise = (t.log() / 4).float()
        emb = R.positional_embedding(c_noise, 128)
        lv = emb @ sd["model.logvar_linear.weight"].t() + sd["model.logvar_linear.bias"]
        assert torch.allclose(logvar.cpu(), lv, atol=1e-5)
        with pytest.raises(AssertionError):
            net(xd, td, fwd_pred_type="score")
        with pytest.raises(ValueError):
            net(xd[:, :2], td)
    with pytest.raises(NotImplementedError):  # grad mode
        net(xd, td, condition=cd)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_sampler_against_reference_golden(nets, golden_dir, mode):
    fx = load(golden_dir, "sampler_full_b2.pt")
    net = nets[mode]
    noise = seeded((2, 3, 32, 32), 0).to(dev())
    cond = fx["cond"].to(dev())
    eps = torch.stack([seeded((2, 3, 32, 32), s) for s in (1, 2, 3)]).to(dev())
    gf = FastGenModel.generator_fn
    amp = torch.bfloat16 if mode == "bf16" else None
    sde = gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="sde", eps=eps, precision_amp=amp)
    check(sde, fx["out_sde"], mode, "4-step sde (graph)")
    sde_eager = gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="sde", eps=eps, use_graph=False)
    assert torch.equal(sde, sde_eager), "graph replay and eager launches must agree bit for bit"
    assert torch.equal(sde, gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="sde", eps=eps))
    check(gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="ode"), fx["out_ode"], mode, "ode")
    check(gf(net, noise, condition=cond, student_sample_steps=1), fx["out_1step"], mode, "1-step")
    check(gf(net, noise, condition=cond, student_sample_steps=2, t_list=[40.0, 1.5, 0.0], student_sample_type="ode"),
          fx["out_tlist"], mode, "custom t_list")
    # graph replay with NEW timesteps reuses the captured graph (timesteps live in device memory)
    captures = _lib.graph_stats()[0]
    check(gf(net, noise, condition=cond, student_sample_steps=2, t_list=[40.0, 1.5, 0.0], student_sample_type="ode"),
          fx["out_tlist"], mode, "custom t_list replay")
    other = gf(net, noise, condition=cond, student_sample_steps=2, t_list=[30.0, 0.7, 0.0], student_sample_type="ode")
    assert _lib.graph_stats()[0] == captures, "a call with the same or with new timesteps captured a new graph"
    assert torch.equal(other, gf(net, noise, condition=cond, student_sample_steps=2, t_list=[30.0, 0.7, 0.0], student_sample_type="ode",
                                 use_graph=False))
    # per-step x0 predictions of the sde trace through the module's forward (generic loop == fused loop)
    with torch.inference_mode():
        tl = net.noise_scheduler.get_t_list(4).to(dev())
        x = net.noise_scheduler.latents(noise, tl[0])
        for i in range(4):
            xp = net(x, tl[i].expand(2), condition=cond, fwd_pred_type="x0")
            check(xp, fx["x_pred_sde"][i], mode, f"x_pred step {i}")
            if i < 3:
                x = net.noise_scheduler.forward_process(xp, eps[i], tl[i + 1].expand(2))
        assert torch.equal(xp, sde)


def test_sampler_batch16_against_oracle(nets, sd):
    """BASELINE configs[0] shape (batch 16, 4-step) against the CPU oracle computed here."""
    B = 16
    noise = seeded((B, 3, 32, 32), 0)
    cond = torch.nn.functional.one_hot(torch.arange(B) % 10, 10).float()
    eps = [seeded((B, 3, 32, 32), s) for s in (1, 2, 3)]
    want = R.generator_fn(sd, R.CIFAR10, noise, cond, 4, sample_type="sde", eps_list=eps)
    for mode in ("fp32", "bf16x3", "bf16"):
        got = FastGenModel.generator_fn(nets[mode], noise.to(dev()), condition=cond.to(dev()), student_sample_steps=4,
                                        student_sample_type="sde", eps=torch.stack(eps).to(dev()))
        check(got, want, mode, f"B=16 sde {mode}")


@pytest.mark.parametrize("B", [1, 3, 5, 18])
def test_ragged_batches(nets, sd, B):
    """Batches that do not fill the 4-image tiles of the 8x8 layers."""
    x, t = seeded((B, 3, 32, 32), 9) * 2, torch.full((B,), 2.5265, dtype=torch.float64)
    cond = torch.nn.functional.one_hot(torch.arange(B) % 10, 10).float()
    with torch.inference_mode():
        want = R.edm_precond_forward(sd, R.CIFAR10, x, t, cond)
        for mode in ("fp32", "bf16x3"):
            check(nets[mode](x.to(dev()), t.to(dev()), condition=cond.to(dev())), want, mode, f"B={B} {mode}")


def test_full_size_properties(nets):
    """BASELINE configs[1] size (batch 512): size-independent properties instead of a CPU run —
    every image is independent of its batch mates (bit-exact vs. the same images in a batch of 16), the sampler is
    deterministic, device RNG is seed-controlled, outputs are finite and O(1)."""
    for mode in ("bf16", "bf16x3", "fp32"):
        net = nets[mode]
        B = 512
        noise = seeded((B, 3, 32, 32), 3).to(dev())
        cond = torch.nn.functional.one_hot(torch.arange(B) % 10, 10).float().to(dev())
        eps = torch.stack([seeded((B, 3, 32, 32), s) for s in (4, 5, 6)]).to(dev())
        gf = FastGenModel.generator_fn
        big = gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="sde", eps=eps)
        assert torch.isfinite(big).all() and 0.05 < big.std().item() < 5
        assert torch.equal(big, gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="sde", eps=eps))
        for lo in (0, 496):
            sl = slice(lo, lo + 16)
            small = gf(net, noise[sl].contiguous(), condition=cond[sl].contiguous(), student_sample_steps=4,
                       student_sample_type="sde", eps=eps[:, sl].contiguous())
            assert torch.equal(big[sl], small), f"{mode}: image result depends on its batch (rows {lo}..{lo + 15})"
        if mode == "bf16":
            a = gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="sde", seed=7)
            b = gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="sde", seed=7)
            c = gf(net, noise, condition=cond, student_sample_steps=4, student_sample_type="sde", seed=8)
            assert torch.equal(a, b) and not torch.equal(a, c)
            # linearity of the re-noising step: x0 prediction of the LAST step does not depend on eps scale being 0
            one = gf(net, noise, condition=cond, student_sample_steps=1)
            assert torch.isfinite(one).all()


def test_weights_repack_on_update(nets, sd):
    """An in-place parameter update (optimizer step / load_state_dict) must reach the packed MFMA copies."""
    net = EDMPrecond(compute_dtype="fp32", **KW)
    net.load_state_dict(sd)
    net = net.to(dev()).eval()
    x, t = seeded((2, 3, 32, 32), 1).to(dev()), torch.tensor([1.0, 2.0], dtype=torch.float64, device=dev())
    with torch.inference_mode():
        a = net(x, t)
    with torch.no_grad():
        net.model._modules["enc"]._modules["32x32_block1"]._modules["conv0"].weight.mul_(0.5)
    with torch.inference_mode():
        b = net(x, t)
    assert not torch.equal(a, b)
    sd2 = {k: v.clone() for k, v in sd.items()}
    net.load_state_dict(sd2)
    with torch.inference_mode():
        assert torch.equal(net(x, t), a)


def test_reference_default_init_runs(nets):
    """Reference-style default init (residual branches x 1e-5): output ~ c_skip * x_t."""
    net = EDMPrecond(compute_dtype="fp32", **KW).to(dev()).eval()
    x, t = seeded((2, 3, 32, 32), 2).to(dev()), torch.tensor([0.5, 0.5], dtype=torch.float64, device=dev())
    with torch.inference_mode():
        out = net(x, t)
    c_skip = 0.25 / (0.25 + 0.25)
    assert torch.allclose(out, c_skip * x, atol=1e-3)


# ---- MeanFlow student (r_timestep, drop_precond, rectified flow): SURVEY 8(f) widening row ---------------------------

KW_MF = {**KW, "label_dim": 0, "augment_dim": 6, "r_timestep": True, "drop_precond": "both", "schedule_type": "rf",
         "net_pred_type": "flow"}


@pytest.fixture(scope="module")
def mf_sd():
    return R.random_state_dict(R.CIFAR10_MEANFLOW, seed=4321)


@pytest.fixture(scope="module")
def mf_nets(mf_sd):
    out = {}
    for mode in ("fp32", "bf16x3", "bf16"):  # bf16x3 = what the module computes outside autocast (DEFAULT_FP32_MODE): held to the fp32 tolerance
        n = EDMPrecond(compute_dtype=mode, **KW_MF)
        n.load_state_dict(mf_sd, strict=True)
        out[mode] = n.to(dev()).eval()
    return out


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_meanflow_forward_against_reference_golden(mf_nets, mf_sd, golden_dir, mode):
    fx = load(golden_dir, "meanflow_full_b2.pt")
    net = mf_nets[mode]
    x = seeded((2, 3, 32, 32), 41).to(dev())
    t, r = fx["t"].to(dev()), fx["r"].to(dev())
    with torch.inference_mode():
        check(net(x, t, r=r, fwd_pred_type="flow"), fx["out"], mode, "u(x, t, r)")
        check(net(x, t, r=r), fx["out"], mode, "default fwd_pred_type = net_pred_type")
        check(net(x, t, r=r, fwd_pred_type="x0"), fx["out_x0"], mode, "flow -> x0 conversion")
        with pytest.raises(ValueError):
            net(x, t)
    # the other preconditioning settings on the same weights
    for dp in (None, "input", "output"):
        nv = EDMPrecond(compute_dtype=mode, **{**KW_MF, "drop_precond": dp})
        nv.load_state_dict(mf_sd, strict=True)
        nv = nv.to(dev()).eval()
        with torch.inference_mode():
            check(nv(x, t, r=r), fx[f"out_drop_{dp}"], mode, f"drop_precond={dp}")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_meanflow_sampler_against_reference_golden(mf_nets, golden_dir, mode):
    fx = load(golden_dir, "meanflow_full_b2.pt")
    net = mf_nets[mode]
    noise = seeded((2, 3, 32, 32), 5).to(dev())
    eps = torch.stack([seeded((2, 3, 32, 32), s) for s in (6, 7, 8)]).to(dev())
    gf = MeanFlowModel.generator_fn
    sde = gf(net, noise, student_sample_steps=4, student_sample_type="sde", eps=eps)
    check(sde, fx["out_sde"], mode, "meanflow 4-step sde (graph)")
    assert torch.equal(sde, gf(net, noise, student_sample_steps=4, student_sample_type="sde", eps=eps, use_graph=False))
    ode = gf(net, noise, student_sample_steps=4, student_sample_type="ode")
    check(ode, fx["out_ode"], mode, "meanflow 4-step ode")
    check(gf(net, noise, student_sample_steps=1, student_sample_type="ode"), fx["out_1step"], mode, "meanflow 1-step")
    check(gf(net, noise, student_sample_steps=2, t_list=[0.999, 0.5, 0.0], student_sample_type="ode"), fx["out_tlist"],
          mode, "meanflow 2-step recommended t_list")
    # the generic per-step loop through the module's forward gives the fused loop's bits
    with torch.inference_mode():
        tl = net.noise_scheduler.get_t_list(4).to(dev())
        x = net.noise_scheduler.latents(noise, tl[0])
        gen = MeanFlowModel._student_sample_loop(net, x, tl, student_sample_type="ode")
    assert torch.equal(gen, ode)
    # FastGenModel's x0 loop is not defined for this network and is refused, not approximated
    with pytest.raises(NotImplementedError):
        net.few_step_sample(noise, None, [0.999, 0.0], loop="x0")
    with pytest.raises(_lib.FastGenAMDError):  # t outside the rectified-flow range
        gf(net, noise, student_sample_steps=1, t_list=[1.5, 0.0], student_sample_type="ode")


def test_meanflow_batch16_against_oracle(mf_nets, mf_sd):
    B = 16
    noise = seeded((B, 3, 32, 32), 0)
    eps = [seeded((B, 3, 32, 32), s) for s in (1, 2, 3)]
    cfg = R.CIFAR10_MEANFLOW
    want_sde = R.generator_fn(mf_sd, cfg, noise, None, 4, sample_type="sde", eps_list=eps, loop="meanflow")
    want_ode = R.generator_fn(mf_sd, cfg, noise, None, 2, sample_type="ode", loop="meanflow")
    for mode in ("fp32", "bf16x3", "bf16"):
        got = MeanFlowModel.generator_fn(mf_nets[mode], noise.to(dev()), student_sample_steps=4,
                                         student_sample_type="sde", eps=torch.stack(eps).to(dev()))
        check(got, want_sde, mode, f"meanflow B=16 sde {mode}")
        got = MeanFlowModel.generator_fn(mf_nets[mode], noise.to(dev()), student_sample_steps=2,
                                         student_sample_type="ode")
        check(got, want_ode, mode, f"meanflow B=16 ode {mode}")


# ---- encoder feature taps (the DMD2 discriminator's inputs, EDM/network.py:525-544) ------------------------------------


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_feature_taps(nets, sd, golden_dir, mode):
    fx = load(golden_dir, "forward_full_b2.pt")
    net = nets[mode]
    x = (seeded((2, 3, 32, 32), 21) * fx["t"].reshape(2, 1, 1, 1).float())
    xd, td, cd = x.to(dev()), fx["t"].to(dev()), fx["cond"].to(dev())
    tr = {}
    with torch.inference_mode():
        want_out = R.edm_precond_forward(sd, R.CIFAR10, x, fx["t"], fx["cond"], trace=tr)
        out, feats = net(xd, td, condition=cd, feature_indices={0, 1, 2})
        early = net(xd, td, condition=cd, feature_indices={0, 1, 2}, return_features_early=True)
        only1 = net(xd, td, condition=cd, feature_indices={1}, return_features_early=True)
        (out_lv, feats_lv), logvar = net(xd, td, condition=cd, feature_indices={2}, return_logvar=True)
        plain = net(xd, td, condition=cd)
    keys = ["model.enc.32x32_block3", "model.enc.16x16_block3", "model.enc.8x8_block3"]
    shapes = [(2, 256, 32, 32), (2, 256, 16, 16), (2, 256, 8, 8)]
    assert [tuple(f.shape) for f in feats] == shapes and len(early) == 3
    for i, k in enumerate(keys):
        check(feats[i], tr[k], mode, f"feature {k} vs oracle")
        # the strided samples recorded from the reference's own forward hooks
        v = feats[i].float().cpu()
        sample = v.reshape(-1)[:: max(1, v.numel() // 4096)][:4096]
        check(sample, fx[f"blk/enc.{k.split('.')[-1]}/sample"], mode, f"feature {k} vs reference sample")
        assert torch.equal(early[i], feats[i])
    assert len(only1) == 1 and torch.equal(only1[0], feats[1])
    assert len(feats_lv) == 1 and torch.equal(feats_lv[0], feats[2]) and logvar.shape == (2, 1)
    assert torch.equal(out, plain) and torch.equal(out_lv, plain)
    check(out, want_out, mode, "output next to the features")
    with torch.inference_mode():
        assert net(xd, td, condition=cd, return_features_early=True) == []
        with pytest.raises(AssertionError):  # the reference's length assert (:543): tap 7 does not exist
            net(xd, td, condition=cd, feature_indices={0, 7}, return_features_early=True)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_teacher_euler_sampler(nets, golden_dir, mode):
    """EDMPrecond.sample (EDM/network.py:976-1026): Euler steps with classifier-free guidance through the module's forward.
    The reference evaluates the network in float64 from the second step on (x is promoted by the division by t); this engine
    computes in fp32 / bf16, which is what the tolerance covers."""
    fx = load(golden_dir, "teacher_sample_b2.pt")
    net = nets[mode]
    noise = seeded((2, 3, 32, 32), 50).to(dev())
    cond = fx["cond"].to(dev())
    with torch.inference_mode():
        out = net.sample(noise, condition=cond, neg_condition=torch.zeros(2, 10, device=dev()), guidance_scale=2.0, num_steps=4)
        assert out.dtype == torch.float64  # same promotion as the reference
        check(out, fx["out_cfg"], mode, "Euler sampler with CFG")
        out = net.sample(noise, condition=cond, guidance_scale=None, num_steps=3)
        check(out, fx["out_plain"], mode, "Euler sampler without guidance")


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_meanflow_full_size_properties(mf_nets, mode):
    """MeanFlow sampler at batch 512: per-image independence (bit-exact vs. the same images in a batch of 16), determinism,
    seed control, and agreement of 'ode' one-step with a hand-written x - t * u(x, t, 0)."""
    net = mf_nets[mode]
    B = 512
    noise = seeded((B, 3, 32, 32), 13).to(dev())
    eps = torch.stack([seeded((B, 3, 32, 32), s) for s in (14, 15, 16)]).to(dev())
    gf = MeanFlowModel.generator_fn
    big = gf(net, noise, student_sample_steps=4, student_sample_type="sde", eps=eps)
    assert torch.isfinite(big).all()
    assert torch.equal(big, gf(net, noise, student_sample_steps=4, student_sample_type="sde", eps=eps))
    for lo in (0, 496):
        sl = slice(lo, lo + 16)
        small = gf(net, noise[sl].contiguous(), student_sample_steps=4, student_sample_type="sde", eps=eps[:, sl].contiguous())
        assert torch.equal(big[sl], small), f"image result depends on its batch (rows {lo}..{lo + 15})"
    a = gf(net, noise, student_sample_steps=4, student_sample_type="sde", seed=7)
    b = gf(net, noise, student_sample_steps=4, student_sample_type="sde", seed=7)
    c = gf(net, noise, student_sample_steps=4, student_sample_type="sde", seed=8)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # one 'ode' step from t = 0.999 to 0 is x - 0.999 * u(x, 0.999, r = 0), x = 0.999 * noise
    one = gf(net, noise, student_sample_steps=1, student_sample_type="ode")
    with torch.inference_mode():
        t = torch.full((B,), 0.999, dtype=torch.float64, device=dev())
        x = net.noise_scheduler.latents(noise, t[0])
        u = net(x, t, r=torch.zeros_like(t), fwd_pred_type="flow")
        assert torch.equal(one, x - t[0].to(x.dtype) * u)
        # scalar / broadcast forms of t and r are accepted like the reference's expand()
        u1 = net(x[:4], torch.tensor(0.999, dtype=torch.float64, device=dev()), r=torch.tensor(0.0, device=dev()))
        assert torch.equal(u1, u[:4])


def test_generic_conv_kernel_path():
    """FASTGEN_AMD_CONV_WS=0 routes every conv through conv_fused_kernel (the kernel that serves fp32 mode and the shapes the
    wave-specialised kernel does not take).  The switch is read once per process, so the bf16 block / forward parity tests run
    again in a child process with it set."""
    import subprocess
    import sys

    if os.environ.get("FASTGEN_AMD_CONV_WS") == "0":
        pytest.skip("already running with the generic kernel")
    env = dict(os.environ, FASTGEN_AMD_CONV_WS="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "(blocks_against or forward_against) and bf16"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# ---- training step, first kernel: conv weight gradient ---------------------------------------------------
def _wgrad(act_nchw, dy_nchw, ks, accumulate_into=None, x3=False):
    """fg_op_conv_wgrad on NHWC bf16 copies of the operands (x3: fg_op_conv_wgrad_f32 on fp32 copies); returns dW
    [Cout, Cin, ks, ks] fp32 (CPU)."""
    L = _lib.lib()
    B, cin, res, _ = act_nchw.shape
    cout = dy_nchw.shape[1]
    st = torch.float32 if x3 else torch.bfloat16
    a = act_nchw.permute(0, 2, 3, 1).contiguous().to(st).cuda()
    d = dy_nchw.permute(0, 2, 3, 1).contiguous().to(st).cuda()
    dw = (torch.zeros(cout, cin, ks, ks) if accumulate_into is None else accumulate_into.clone()).float().cuda()
    nbytes = L.fg_op_conv_wgrad_workspace_bytes(B, res, cin, cout, ks)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    fn = L.fg_op_conv_wgrad_f32 if x3 else L.fg_op_conv_wgrad
    _lib.check(fn(a.data_ptr(), d.data_ptr(), dw.data_ptr(), B, res, cin, cout, ks,
                  0 if accumulate_into is None else 1, ws.data_ptr(), nbytes, None))
    torch.cuda.synchronize()
    return dw.cpu()


@pytest.mark.parametrize("B,res,cin,cout,ks", [(3, 32, 64, 128, 3), (2, 16, 96, 256, 3), (5, 8, 32, 128, 3), (3, 32, 128, 256, 1),
                                               (2, 16, 256, 128, 1), (4, 8, 384, 128, 1)])
def test_conv_wgrad_split_bf16_against_oracle(B, res, cin, cout, ks):
    """The bf16x3 weight gradient on FULL fp32 operands (no pre-rounding) vs fp32 autograd: relative L2 <= 2e-5 and
    max |err| <= 5e-5 of the largest entry (2^-17 per product; the bf16 kernel on the same data is at 4e-3)."""
    g = torch.Generator().manual_seed(res * 1000 + cin + ks + 7)
    act = torch.randn((B, cin, res, res), generator=g)
    dy = torch.randn((B, cout, res, res), generator=g)
    want = R.conv_weight_grad(act.double(), dy.double(), ks).float()
    got = _wgrad(act, dy, ks, x3=True)
    rel = float((got - want).norm() / want.norm())
    assert rel <= 2e-5 and (got - want).abs().max() <= 5e-5 * want.abs().max(), (rel, float((got - want).abs().max() / want.abs().max()))
    assert torch.equal(got, _wgrad(act, dy, ks, x3=True))
    base = torch.randn(want.shape, generator=g)
    acc = _wgrad(act, dy, ks, accumulate_into=base, x3=True)
    assert (acc - (base + got)).abs().max() <= 1e-5 * want.abs().max()


@pytest.mark.parametrize("B,res,cin,cout,ks", [(3, 32, 64, 128, 3), (2, 16, 96, 256, 3), (5, 8, 32, 128, 3), (1, 8, 64, 256, 3),
                                               (3, 32, 128, 256, 1), (2, 16, 256, 128, 1), (4, 8, 384, 128, 1)])
def test_conv_wgrad_against_oracle(B, res, cin, cout, ks):
    """Weight gradient on the matrix cores (bf16 operands, fp32 accumulation) vs autograd on the same bf16-rounded operands
    in fp32: only the summation order differs — max |err| <= 2e-5 of the largest entry."""
    g = torch.Generator().manual_seed(res * 1000 + cin + ks)
    act = torch.randn((B, cin, res, res), generator=g).to(torch.bfloat16).float()
    dy = torch.randn((B, cout, res, res), generator=g).to(torch.bfloat16).float()
    want = R.conv_weight_grad(act, dy, ks)
    got = _wgrad(act, dy, ks)
    assert got.shape == want.shape
    assert (got - want).abs().max() <= 2e-5 * want.abs().max(), float((got - want).abs().max() / want.abs().max())
    # deterministic, and accumulate adds to what is there
    assert torch.equal(got, _wgrad(act, dy, ks))
    base = torch.randn(want.shape, generator=g)
    acc = _wgrad(act, dy, ks, accumulate_into=base)
    assert (acc - (base + got)).abs().max() <= 1e-5 * want.abs().max()


def test_conv_wgrad_reference_golden_and_full_size(golden_dir):
    """(1) The reference's own Conv2d weight gradient (tests/golden/backward_conv.pt): fp32 operands are rounded to bf16 on
    the way in, so the tolerance is bf16's (relative L2 <= 1e-2).  (2) Training-size batch, 256 -> 256 at 32x32: additive
    over a batch split (size-independent property) and equal to the oracle on a slice of output channels."""
    fx = torch.load(os.path.join(golden_dir, "backward_conv.pt"), weights_only=True)
    for ks in (3, 1):
        B, cin, cout, res, _ = fx[f"k{ks}/shape"].tolist()
        x = torch.randn((B, cin, res, res), generator=torch.Generator().manual_seed(53 + ks))
        dy = torch.randn((B, cout, res, res), generator=torch.Generator().manual_seed(54 + ks))
        got, want = _wgrad(x, dy, ks), fx[f"k{ks}/weight_grad"]
        assert ((got - want).norm() / want.norm()) <= 1e-2
    g = torch.Generator().manual_seed(99)
    B = 64
    act = torch.randn((B, 256, 32, 32), generator=g).to(torch.bfloat16).float()
    dy = torch.randn((B, 256, 32, 32), generator=g).to(torch.bfloat16).float()
    full = _wgrad(act, dy, 3)
    halves = _wgrad(act[: B // 2], dy[: B // 2], 3) + _wgrad(act[B // 2:], dy[B // 2:], 3)
    assert (full - halves).abs().max() <= 2e-5 * full.abs().max()
    want = R.conv_weight_grad(act[:, :32], dy[:, :8], 3)  # [8, 32, 3, 3] corner of the full gradient
    assert (full[:8, :32] - want).abs().max() <= 2e-5 * full.abs().max()


def test_conv_wgrad_rejects_bad_arguments():
    L = _lib.lib()
    assert L.fg_op_conv_wgrad_workspace_bytes(2, 32, 48, 128, 3) == 0  # cin % 32
    x = torch.zeros(16, device="cuda")
    with pytest.raises(_lib.FastGenAMDError):
        _lib.check(L.fg_op_conv_wgrad(x.data_ptr(), x.data_ptr(), x.data_ptr(), 2, 32, 64, 100, 3, 0, x.data_ptr(), 64, None))
    with pytest.raises(_lib.FastGenAMDError):  # workspace too small
        _lib.check(L.fg_op_conv_wgrad(x.data_ptr(), x.data_ptr(), x.data_ptr(), 2, 32, 64, 128, 3, 0, x.data_ptr(), 64, None))


# ---- training step, block level: UNetBlock backward --------------------------------------------------------
BWD_BLOCKS = {"enc_first": "32x32_block0", "enc_plain": "8x8_block1", "dec_cat512": "16x16_block1", "dec_cat384": "32x32_block4"}


# per-tensor relative L2 of a block's gradients: bf16 activations / activation gradients, or fp32 tensors with split-bf16 products
BWD_TOL = {"bf16": dict(block=2e-2, norm=2e-2, sample=3e-2), "bf16x3": dict(block=1e-4, norm=1e-4, sample=2e-4)}


def _block_backward_hip(net, sd, b, bi, key, names, x, emb, dout):
    """fg_edm_run_block_backward through the C ABI with the block's parameter gradients bound; x, dout NCHW fp32 on the CPU.  Returns
    {"dx", "demb", <parameter name without the block's key>: gradient} on the CPU."""
    L = _lib.lib()
    bs, rin = x.shape[0], x.shape[2]
    with torch.inference_mode():
        dt, h = net._engine(dev())
        c2 = b.skip_from or 0
        c1 = b.cin - c2
        x1 = nhwc(x[:, :c1]).to(dev())
        x2 = nhwc(x[:, c1:]).to(dev()) if c2 else None
        grads = {k: torch.zeros_like(sd[k], device=dev()) for k in names}
        for k, g in grads.items():
            _lib.check(L.fg_edm_bind_grad(h, k.encode(), g.data_ptr(), g.numel()))
        try:
            dx1 = torch.full((bs, rin, rin, c1), float("nan"), device=dev())  # overwritten: an element left out shows
            dx2 = torch.full((bs, rin, rin, max(c2, 1)), float("nan"), device=dev())
            demb = torch.zeros(bs, 512, device=dev())
            nbytes = L.fg_edm_block_backward_workspace_bytes(h, bi, bs)
            assert nbytes > 0
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
            # device copies held in names: a temporary's memory returns to the caching allocator as soon as data_ptr() has been
            # taken, and the next temporary may be carved from the same block (it was: a stale emb pointer read dout's bytes
            # whenever three networks' worth of small allocations had shaped the free lists that way)
            emb_d, dout_d = emb.to(dev()), nhwc(dout).to(dev())
            _lib.check(L.fg_edm_run_block_backward(h, bi, x1.data_ptr(), c1, x2.data_ptr() if c2 else None, c2,
                                                   emb_d.data_ptr(), dout_d.data_ptr(), dx1.data_ptr(),
                                                   dx2.data_ptr() if c2 else None, demb.data_ptr(), bs, ws.data_ptr(), nbytes, None))
            torch.cuda.synchronize()
        finally:
            for k in grads:
                _lib.check(L.fg_edm_bind_grad(h, k.encode(), None, 0))
    dx = torch.cat([nchw(dx1.cpu()), nchw(dx2.cpu())], 1) if c2 else nchw(dx1.cpu())
    got = {"dx": dx, "demb": demb.cpu(), **{k[len(key) + 1:]: g.cpu() for k, g in grads.items()}}
    return got


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("case", ["enc_first", "enc_plain", "dec_cat512", "dec_cat384", "enc_down", "dec_up", "enc_attn", "dec_in0",
                                  "dec_cat_attn"])
def test_block_backward_against_reference_golden(nets, sd, golden_dir, case, mode):
    """d/dx, d/demb and every parameter gradient of one UNetBlock against (1) autograd through the oracle in fp32 on the same
    operands — relative L2 per tensor <= 2e-2 in the bf16 mode (bf16 activations and activation gradients), <= 1e-4 in the
    bf16x3 mode (fp32 tensors, the reference's training precision) — and (2) the norms / strided samples recorded from the
    reference's own module under autograd (tests/golden/blocks_backward.pt)."""
    fx = load(golden_dir, "blocks_backward.pt")
    net = nets[mode]
    tol = BWD_TOL[mode]
    L = _lib.lib()
    enc, dec = R.layout(R.CIFAR10)
    blocks = [b for b in enc + dec if b.kind == "block"]
    key = fx[f"{case}/key"]
    bi = [i for i, b in enumerate(blocks) if b.key == key][0]
    b = blocks[bi]
    bs = int(fx[f"{case}/bs"])
    s_x, s_e, s_d = fx[f"{case}/seeds"].tolist()
    rin = b.res * 2 if b.down else (b.res // 2 if b.up else b.res)
    x = seeded((bs, b.cin, rin, rin), s_x)
    emb = seeded((bs, 512), s_e) * 0.5
    dout = seeded((bs, b.cout, b.res, b.res), s_d)
    # ---- oracle: autograd through the CPU restatement --------------------------------------------------------------
    names = [k for k in sd if k.startswith(key + ".") and "resample_filter" not in k]  # buffers carry no gradient
    sdg = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    xo, eo = x.clone().requires_grad_(True), emb.clone().requires_grad_(True)
    with torch.enable_grad():
        R.unet_block(sdg, b, xo, eo).backward(dout)
    want = {"dx": xo.grad, "demb": eo.grad, **{k[len(key) + 1:]: sdg[k].grad for k in names}}
    # ---- HIP path through the C ABI --------------------------------------------------------------------------------------
    got = _block_backward_hip(net, sd, b, bi, key, names, x, emb, dout)
    assert set(got) == set(want)
    for n in sorted(want):
        rel = float((got[n] - want[n]).norm() / want[n].norm())
        assert rel <= tol["block"], (case, mode, n, rel)
        # the reference's own numbers: norm and strided sample
        gn, gs = fx[f"{case}/{n}/norm"], fx[f"{case}/{n}/sample"]
        flat = got[n].reshape(-1)
        smp = flat[:: max(1, flat.numel() // 4096)][:4096]
        assert abs(float(flat.double().norm()) / float(gn) - 1) <= tol["norm"], (case, mode, n)
        assert float((smp - gs).norm() / gs.norm()) <= tol["sample"], (case, mode, n)


# Batch 5 puts a second image on batch lane 0 of gn_bwd_group_param_kernel / batchsum_add_kernel (the golden cases run at batch 1 or 2);
# the 32x32 cases run at batch 3 to keep the fp64 oracle to a few seconds.
SLICE_BATCH = {"enc_plain": 5, "enc_attn": 5, "dec_cat512": 5, "dec_cat_attn": 5, "dec_in0": 5, "enc_down": 5, "enc_first": 3, "dec_cat384": 3,
               "dec_up": 3}
_SLICE_ORACLE = {}


def _slice_oracle(sd, golden_dir, case):
    """(block, index, key, names, x, emb, dout, fp64 autograd gradients) of one case, computed once for both modes."""
    if case not in _SLICE_ORACLE:
        fx = load(golden_dir, "blocks_backward.pt")
        enc, dec = R.layout(R.CIFAR10)
        blocks = [b for b in enc + dec if b.kind == "block"]
        key = fx[f"{case}/key"]
        bi = [i for i, b in enumerate(blocks) if b.key == key][0]
        b = blocks[bi]
        bs = SLICE_BATCH[case]
        rin = b.res * 2 if b.down else (b.res // 2 if b.up else b.res)
        x, emb, dout = seeded((bs, b.cin, rin, rin), 9100 + bi), seeded((bs, 512), 9200 + bi) * 0.5, seeded((bs, b.cout, b.res, b.res), 9300 + bi)
        names = [k for k in sd if k.startswith(key + ".") and "resample_filter" not in k]
        sdg = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items() if k.startswith(key + ".")}
        for k in names:
            sdg[k].requires_grad_(True)
        xo, eo = x.double().requires_grad_(True), emb.double().requires_grad_(True)
        with torch.enable_grad():
            R.unet_block(sdg, b, xo, eo).backward(dout.double())
        want = {"dx": xo.grad, "demb": eo.grad, **{k[len(key) + 1:]: sdg[k].grad for k in names}}
        _SLICE_ORACLE[case] = (b, bi, key, names, x, emb, dout, want)
    return _SLICE_ORACLE[case]


def _slices(name, t):
    """{slicing: dims reduced} of one gradient tensor: dx per image, pixel row, pixel column and 8-channel octet; a conv weight per
    output channel and per tap; demb per image."""
    if name == "dx":
        B, C, H, W = t.shape
        o = t.reshape(B, C // 8, 8, H, W)
        return {"image": (t, (1, 2, 3)), "row": (t, (0, 1, 3)), "column": (t, (0, 1, 2)), "octet": (o, (0, 2, 3, 4))}
    if name == "demb":
        return {"image": (t, (1,))}
    if t.dim() == 4:
        return {"cout": (t, (1, 2, 3)), "tap": (t, (0, 1))}
    return {}


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("case", sorted(SLICE_BATCH))
def test_block_backward_per_slice_against_fp64_autograd(nets, sd, golden_dir, case, mode):
    """fg_edm_run_block_backward at batch 5 (3 at 32x32) against fp64 autograd through the oracle's UNetBlock: BWD_TOL's relative L2 per
    tensor AND per slice of every gradient - a wrong value confined to one image, one border row or column, one octet, one output
    channel or one tap moves the whole tensor's relative L2 only by the root of its share.  A slice is skipped only if its reference
    norm is below 1e-3 of the tensor's RMS times the root of the slice size (at most 2 % of a slicing); per-channel vectors are
    compared per entry against tol * max|want|."""
    b, bi, key, names, x, emb, dout, want = _slice_oracle(sd, golden_dir, case)
    tol = BWD_TOL[mode]["block"]
    got = _block_backward_hip(nets[mode], sd, b, bi, key, names, x, emb, dout)
    assert set(got) == set(want)
    worst = {}
    for n in sorted(want):
        g, w = got[n].double(), want[n]
        assert torch.isfinite(g).all(), (case, mode, n)
        rel = float((g - w).norm() / w.norm())
        assert rel <= tol, (case, mode, n, rel)
        if w.dim() == 1:
            e = float((g - w).abs().max() / w.abs().max())
            worst["entry"] = max(worst.get("entry", 0.0), e)
            assert e <= tol, (case, mode, n, "entry", e)
            continue
        rms = float(w.pow(2).mean().sqrt())
        for kind, (wv, dims) in _slices(n, w).items():
            gv = _slices(n, g)[kind][0]
            num, den = (gv - wv).pow(2).sum(dims).sqrt(), wv.pow(2).sum(dims).sqrt()
            size = wv.numel() // den.numel()
            keep = den >= 1e-3 * rms * size ** 0.5
            assert int((~keep).sum()) <= 0.02 * den.numel(), (case, mode, n, kind, "slices skipped", int((~keep).sum()), den.numel())
            r = float((num[keep] / den[keep]).max())
            worst[kind] = max(worst.get(kind, 0.0), r)
            assert r <= tol, (case, mode, n, kind, r, int((num / den.clamp_min(1e-300) * keep).argmax()))
    print(f"SLICES {case} {mode} " + " ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())))


# ---- training step, whole network: EDMPrecond backward ------------------------------------------------------
def _net_backward(net, sd, x, t, cond, dout):
    """fg_edm_backward through the C ABI with every parameter gradient bound; returns (out, {name: grad}) on the CPU."""
    L = _lib.lib()
    B = x.shape[0]
    with torch.inference_mode():
        dt, h = net._engine(dev())
        names = [k for k, v in sd.items() if v.is_floating_point() and "resample_filter" not in k]
        grads = {k: torch.zeros_like(sd[k], device=dev()) for k in names}
        for k, g in grads.items():
            _lib.check(L.fg_edm_bind_grad(h, k.encode(), g.data_ptr(), g.numel()))
        try:
            nbytes = L.fg_edm_backward_workspace_bytes(h, B)
            assert nbytes > 0
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
            out = torch.empty_like(x, device=dev())
            xd, td, cd, dd = x.to(dev()), t.to(dev()), cond.to(dev()).contiguous(), dout.to(dev())
            _lib.check(L.fg_edm_backward(h, xd.data_ptr(), td.data_ptr(), None, cd.data_ptr(), dd.data_ptr(), out.data_ptr(), 0, B,
                                         ws.data_ptr(), nbytes, None))
            torch.cuda.synchronize()
        finally:
            for k in grads:
                _lib.check(L.fg_edm_bind_grad(h, k.encode(), None, 0))
    return out.cpu(), {k: g.cpu() for k, g in grads.items()}


def test_network_backward_split_bf16_against_reference_golden(nets, sd, golden_dir):
    """The reference trains this config in fp32 (configs/config.py:167-169).  Every parameter gradient of EDMPrecond in the
    bf16x3 mode (fp32 tensors, split-bf16 products; no autocast) against the reference's autograd (full_backward_b2.pt):
    relative L2 of the sampled entries <= 1e-3 for EVERY tensor, norm within 1e-3."""
    fx = load(golden_dir, "full_backward_b2.pt")
    names = open(os.path.join(golden_dir, "full_backward_names.txt")).read().split()
    t, cond = fx["t"], fx["cond"]
    x = seeded((2, 3, 32, 32), 21) * t.reshape(2, 1, 1, 1).float()
    dout = seeded((2, 3, 32, 32), 401)
    out, grads = _net_backward(nets["bf16x3"], sd, x, t, cond, dout)
    check(out, fx["out"], "bf16x3", "forward value of fg_edm_backward")
    errs = []
    for n in names:
        g = grads[n].reshape(-1)
        smp = g[:: max(1, g.numel() // 512)][:512]
        want_s, want_n = fx[f"{n}/sample"], float(fx[f"{n}/norm"])
        errs.append((float((smp - want_s).norm() / want_s.norm().clamp_min(1e-20)), n))
        assert abs(float(g.double().norm()) / want_n - 1) <= 1e-3, n
    errs.sort(reverse=True)
    print("bf16x3 backward, worst relative errors:", errs[:3], "median", errs[len(errs) // 2][0])
    assert errs[0][0] <= 1e-3, errs[:5]


def test_network_backward_against_reference_golden(nets, sd, golden_dir):
    """Every parameter gradient of EDMPrecond (bf16 compute) for dL/dout = seeded noise, against the norms and strided samples
    recorded from the reference under autograd (tests/golden/full_backward_b2.pt).  Tolerance: relative L2 of the sampled
    entries <= 1e-1 for every tensor, <= 6e-2 for 95 % of them, median <= 4e-2, norm within 3 % per tensor (bf16 activations and
    gradients through up to 36 blocks: accumulated rounding noise, quantified in DESIGN.md section 8); the forward
    value returned alongside matches the reference forward to the bf16 forward tolerance."""
    fx = load(golden_dir, "full_backward_b2.pt")
    names = open(os.path.join(golden_dir, "full_backward_names.txt")).read().split()
    t, cond = fx["t"], fx["cond"]
    x = seeded((2, 3, 32, 32), 21) * t.reshape(2, 1, 1, 1).float()
    dout = seeded((2, 3, 32, 32), 401)
    out, grads = _net_backward(nets["bf16"], sd, x, t, cond, dout)
    check(out, fx["out"], "bf16", "forward value of fg_edm_backward")
    assert len(names) == 418
    errs = []
    for n in names:
        g = grads[n].reshape(-1)
        smp = g[:: max(1, g.numel() // 512)][:512]
        want_s, want_n = fx[f"{n}/sample"], float(fx[f"{n}/norm"])
        errs.append((float((smp - want_s).norm() / want_s.norm().clamp_min(1e-20)), n))
        assert abs(float(g.double().norm()) / want_n - 1) <= 3e-2, n
    errs.sort(reverse=True)
    worst = errs[0]
    # accumulated bf16 rounding (see the MeanFlow variant of this test below): every tensor <= 1e-1, 95 % <= 6e-2, median <= 4e-2
    assert errs[0][0] <= 1e-1, errs[:5]
    assert errs[len(errs) // 20][0] <= 6e-2, errs[: len(errs) // 20 + 1]
    assert errs[len(errs) // 2][0] <= 4e-2
    # parameters the forward never reads get no gradient
    for n in ("model.map_augment.weight", "model.logvar_linear.weight", "model.logvar_linear.bias"):
        assert float(grads[n].abs().max()) == 0.0
    print("worst relative error:", worst)


def test_module_autograd_through_the_hip_backward(nets, golden_dir):
    """loss.backward() through the drop-in module: parameter .grad tensors come from fg_edm_backward and match the reference's
    autograd (same fixture and tolerance as the C-ABI test); a second backward accumulates; unsupported requests raise."""
    fx = load(golden_dir, "full_backward_b2.pt")
    names = open(os.path.join(golden_dir, "full_backward_names.txt")).read().split()
    net = nets["bf16"]
    t, cond = fx["t"].to(dev()), fx["cond"].to(dev())
    x = (seeded((2, 3, 32, 32), 21) * fx["t"].reshape(2, 1, 1, 1).float()).to(dev())
    dout = seeded((2, 3, 32, 32), 401).to(dev())
    params = dict(net.named_parameters())
    try:
        net.zero_grad(set_to_none=True)
        out = net(x, t, condition=cond, fwd_pred_type="x0")
        assert out.requires_grad
        check(out, fx["out"], "bf16", "forward under autograd")
        (out * dout).sum().backward()
        for n in names[::7] + ["model.enc.32x32_conv.weight", "model.map_label.weight", "model.dec.32x32_aux_conv.weight"]:
            g = params[n].grad.detach().cpu().reshape(-1)
            smp = g[:: max(1, g.numel() // 512)][:512]
            want = fx[f"{n}/sample"]
            assert float((smp - want).norm() / want.norm().clamp_min(1e-20)) <= 8e-2, n
        # parameters the call never read stay out of the graph, as in the reference (AdamW must not decay them)
        assert params["model.map_augment.weight"].grad is None and params["model.logvar_linear.weight"].grad is None
        first = params["model.enc.16x16_block1.conv1.weight"].grad.clone()
        (net(x, t, condition=cond, fwd_pred_type="x0") * dout).sum().backward()
        second = params["model.enc.16x16_block1.conv1.weight"].grad
        assert torch.allclose(second, 2 * first, rtol=1e-5, atol=1e-6 * float(first.abs().max()))  # deterministic and accumulated
        # two forwards before the first backward: the older call's kept state is gone, its backward recomputes the forward
        net.zero_grad(set_to_none=True)
        o1 = net(x, t, condition=cond, fwd_pred_type="x0")
        o2 = net(x * 0.5, t, condition=cond, fwd_pred_type="x0")
        (o1 * dout).sum().backward()
        again = params["model.enc.16x16_block1.conv1.weight"].grad.clone()
        assert torch.allclose(again, first, rtol=1e-5, atol=1e-6 * float(first.abs().max()))
        (o2 * dout).sum().backward()
        assert torch.isfinite(params["model.enc.16x16_block1.conv1.weight"].grad).all()
        with pytest.raises(NotImplementedError):
            nets["fp32"](x, t, condition=cond)  # the backward pass exists in the bf16 mode only
        # the uncertainty head used by the sCM-family losses trains alongside (return_logvar under autograd)
        net.zero_grad(set_to_none=True)
        o, lv = net(x, t, condition=cond, fwd_pred_type="x0", return_logvar=True)
        assert lv.shape == (2, 1) and lv.requires_grad
        ((o * dout).sum() + lv.sum()).backward()
        assert float(params["model.logvar_linear.weight"].grad.abs().max()) > 0
        # a conversion after the network stays differentiable (eps prediction from the x0 network)
        net.zero_grad(set_to_none=True)
        net(x, t, condition=cond, fwd_pred_type="eps").square().mean().backward()
        assert torch.isfinite(params["model.dec.32x32_aux_conv.weight"].grad).all()
    finally:
        net.zero_grad(set_to_none=True)


def test_backward_releases_gradients_in_three_stages(nets, golden_dir):
    """The module's backward is three autograd nodes (decoder + head, encoder + stem, embedding MLP: fg_edm_backward_part), so a
    data-parallel wrapper sees the decoder's gradients while the encoder is still being differentiated (torch DDP reduces a
    bucket once the hooks of all its parameters have fired, fastgen/utils/distributed/ddp.py:44-72).  Checked here: the order in
    which the parameters' post-accumulate hooks fire, and that the staged pass produces the gradients of the single call."""
    fx = load(golden_dir, "full_backward_b2.pt")
    net = nets["bf16"]
    t, cond = fx["t"].to(dev()), fx["cond"].to(dev())
    x = (seeded((2, 3, 32, 32), 21) * fx["t"].reshape(2, 1, 1, 1).float()).to(dev())
    dout = seeded((2, 3, 32, 32), 401).to(dev())
    order, handles = [], []
    for n, p in net.named_parameters():
        handles.append(p.register_post_accumulate_grad_hook(lambda p_, n=n: order.append(n)))
    try:
        net.zero_grad(set_to_none=True)
        (net(x, t, condition=cond, fwd_pred_type="x0") * dout).sum().backward()
    finally:
        for hd in handles:
            hd.remove()
    stage = [0 if n.startswith("model.dec.") else (1 if n.startswith("model.enc.") else 2) for n in order]
    assert stage == sorted(stage) and set(stage) == {0, 1, 2}, "decoder, then encoder, then embedding parameters"
    assert len(order) == 418 == len(set(order))  # every parameter the call reads (421 minus map_augment and logvar_linear), once
    # same numbers as the one-call backward of the C ABI (fg_edm_backward = all three parts at once)
    _, want = _net_backward(net, {k: v for k, v in net.state_dict().items()}, x.cpu(), fx["t"], fx["cond"], dout.cpu())
    for n in ("model.dec.32x32_block2.conv1.weight", "model.enc.16x16_block1.affine.weight", "model.enc.32x32_conv.weight",
              "model.map_layer0.weight", "model.dec.8x8_in0.qkv.bias", "model.enc.16x16_down.conv0.bias"):
        assert torch.equal(dict(net.named_parameters())[n].grad.cpu(), want[n]), n
    net.zero_grad(set_to_none=True)


def test_module_autograd_at_the_reference_training_precision(sd, golden_dir):
    """What a `_target_`-swapped fp32 training config does (configs/config.py:167-169: precision float32, no AMP): the module
    as constructed by the config (no compute_dtype, no autocast) under loss.backward().  The call runs in the bf16x3 mode; every
    sampled parameter gradient and d/dx_t match the reference's autograd (full_backward_b2.pt) to relative L2 <= 1e-3, feature
    taps + input gradient of the GAN branch included; .grad stays None for the parameters the call never read."""
    fx = load(golden_dir, "full_backward_b2.pt")
    names = open(os.path.join(golden_dir, "full_backward_names.txt")).read().split()
    net = EDMPrecond(**KW)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev()).train()
    t, cond = fx["t"].to(dev()), fx["cond"].to(dev())
    x0 = seeded((2, 3, 32, 32), 21) * fx["t"].reshape(2, 1, 1, 1).float()
    dout = seeded((2, 3, 32, 32), 401).to(dev())
    params = dict(net.named_parameters())

    def rel(a, b):
        return float((a.detach().cpu().float() - b).norm() / b.norm().clamp_min(1e-20))

    def smp(g):
        g = g.detach().cpu().reshape(-1)
        return g[:: max(1, g.numel() // 512)][:512]

    assert not torch.is_autocast_enabled()
    xg = x0.clone().to(dev()).requires_grad_(True)
    out = net(xg, t, condition=cond, fwd_pred_type="x0")
    check(out, fx["out"], "bf16x3", "forward under autograd, default precision")
    out.backward(dout)
    worst = max((rel(smp(params[n].grad), fx[f"{n}/sample"]), n) for n in names)
    assert worst[0] <= 1e-3, worst
    assert rel(xg.grad, fx["gan/dx_out"]) <= 1e-3
    assert params["model.map_augment.weight"].grad is None and params["model.logvar_linear.weight"].grad is None
    # GAN branch: taps returned early, gradient arriving at the taps only
    dfs = [seeded(s, 410 + i).to(dev()) for i, s in enumerate([(2, 256, 32, 32), (2, 256, 16, 16), (2, 256, 8, 8)])]
    net.zero_grad(set_to_none=True)
    xg = x0.clone().to(dev()).requires_grad_(True)
    feats = net(xg, t, condition=cond, return_features_early=True, feature_indices={0, 1, 2})
    for i, f in enumerate(feats):
        assert rel(smp(f), fx[f"gan/feat{i}/sample"]) <= 2e-5
    torch.autograd.backward(feats, dfs)
    assert rel(xg.grad, fx["gan/dx_early"]) <= 1e-3
    for n in fx["gan/probe_names"]:
        assert rel(smp(params[n].grad), fx[f"gan/early/{n}/sample"]) <= 1e-3, n
    # forward-mode derivative in the same mode: <jvp(v), dout> == <v, dx>
    v = seeded((2, 3, 32, 32), 133).to(dev())
    _, jv = net.jvp(x0.to(dev()), t, v, condition=cond)
    lhs, rhs = float((jv * dout).sum()), float((v.cpu() * fx["gan/dx_out"]).sum())
    assert abs(lhs - rhs) <= 1e-3 * abs(rhs) + 1e-4, (lhs, rhs)


def test_sigma_shift_follows_train_eval_mode(sd, golden_dir):
    """sigma_shift enters precond_output in eval mode only (EDM/network.py:956).  Module with sigma_shift = 0.003 against the
    reference in both modes (tests/golden/sigma_shift_b2.pt): outputs in every compute mode, d<out, dout>/dx_t through the
    bf16 backward, the forward-mode derivative along x consistent with it, and the fused sampler (eval mode by construction)."""
    fx = load(golden_dir, "sigma_shift_b2.pt")
    t, cond = fx["t"].to(dev()), fx["cond"].to(dev())
    x = (seeded((2, 3, 32, 32), 131) * (0.25 + fx["t"].reshape(2, 1, 1, 1).float())).to(dev())
    dout = seeded((2, 3, 32, 32), 132).to(dev())
    for mode in ("fp32", "bf16x3", "bf16"):
        net = EDMPrecond(compute_dtype=mode, **{**KW, "sigma_shift": float(fx["sigma_shift"])})
        net.load_state_dict(sd, strict=True)
        net = net.to(dev())
        for tr in (False, True, False):  # and back: the flag is per call, not sticky
            net.train(tr)
            with torch.no_grad():
                check(net(x, t, condition=cond, fwd_pred_type="x0"), fx["out_train" if tr else "out_eval"], mode, f"{mode} train={tr}")
        if mode == "bf16":
            net.requires_grad_(False)
            for tr in (False, True):
                net.train(tr)
                xg = x.clone().requires_grad_(True)
                net(xg, t, condition=cond, fwd_pred_type="x0").backward(dout)
                want = fx["dx_train" if tr else "dx_eval"]
                r = float((xg.grad.cpu() - want).norm() / want.norm())
                assert r <= 8e-2, (tr, r)
                # forward mode agrees: <jvp(v), dout> == <v, dx>
                v = seeded((2, 3, 32, 32), 133).to(dev())
                _, jv = net.jvp(x, t, v, condition=cond)
                lhs, rhs = float((jv * dout).sum()), float((v.cpu() * want).sum())
                assert abs(lhs - rhs) <= 5e-2 * abs(rhs) + 1e-3, (tr, lhs, rhs)
            net.train(True)  # generator_fn switches to eval for the call and restores (utils/basic_utils.py:89-125)
            noise = seeded((2, 3, 32, 32), 7).to(dev())
            a = FastGenModel.generator_fn(net, noise, condition=cond, student_sample_steps=2, student_sample_type="ode")
            assert net.training
            net.eval()
            b = FastGenModel.generator_fn(net, noise, condition=cond, student_sample_steps=2, student_sample_type="ode")
            assert torch.equal(a, b)


def test_module_autograd_feature_taps_and_input_gradient(nets, golden_dir):
    """The gradient paths of DMD2's GAN branch (dmd2.py:137-146): the frozen teacher's feature taps feed the discriminator and
    the loss is differentiated back to the teacher's INPUT.  d out / d x_t, early-returned taps -> x_t and encoder parameters,
    and prediction + bottleneck tap together, against the reference's autograd (tests/golden/full_backward_b2.pt, 'gan/*').
    Tolerance: relative L2 <= 8e-2 (bf16 activations and gradients)."""
    fx = load(golden_dir, "full_backward_b2.pt")
    net = nets["bf16"]
    t, cond = fx["t"].to(dev()), fx["cond"].to(dev())
    x0 = seeded((2, 3, 32, 32), 21) * fx["t"].reshape(2, 1, 1, 1).float()
    dout = seeded((2, 3, 32, 32), 401).to(dev())
    dfs = [seeded(s, 410 + i).to(dev()) for i, s in enumerate([(2, 256, 32, 32), (2, 256, 16, 16), (2, 256, 8, 8)])]
    params = dict(net.named_parameters())

    def rel(a, b):
        return float((a.detach().cpu().float() - b).norm() / b.norm())

    def smp(g):
        g = g.detach().cpu().reshape(-1)
        return g[:: max(1, g.numel() // 512)][:512]

    try:
        # (a) frozen network, gradient with respect to the input only
        net.requires_grad_(False)
        xg = x0.clone().to(dev()).requires_grad_(True)
        net(xg, t, condition=cond, fwd_pred_type="x0").backward(dout)
        assert rel(xg.grad, fx["gan/dx_out"]) <= 8e-2, rel(xg.grad, fx["gan/dx_out"])
        assert all(p.grad is None for p in net.parameters())
        # (b) taps returned early
        net.requires_grad_(True)
        net.zero_grad(set_to_none=True)
        xg = x0.clone().to(dev()).requires_grad_(True)
        feats = net(xg, t, condition=cond, return_features_early=True, feature_indices={0, 1, 2})
        assert [tuple(f.shape) for f in feats] == [(2, 256, 32, 32), (2, 256, 16, 16), (2, 256, 8, 8)]
        for i, f in enumerate(feats):
            assert rel(smp(f), fx[f"gan/feat{i}/sample"]) <= 1e-2
        torch.autograd.backward(feats, dfs)
        assert rel(xg.grad, fx["gan/dx_early"]) <= 8e-2, rel(xg.grad, fx["gan/dx_early"])
        for n in fx["gan/probe_names"]:
            assert rel(smp(params[n].grad), fx[f"gan/early/{n}/sample"]) <= 8e-2, n
        g = params["model.dec.8x8_in0.conv0.weight"].grad  # nothing downstream of the encoder took part
        assert g is None or float(g.abs().max()) == 0.0
        # (c) prediction and the bottleneck tap together
        net.zero_grad(set_to_none=True)
        xg = x0.clone().to(dev()).requires_grad_(True)
        o, fe = net(xg, t, condition=cond, feature_indices={2}, fwd_pred_type="x0")
        torch.autograd.backward([o, fe[0]], [dout, dfs[2]])
        assert rel(xg.grad, fx["gan/dx_both"]) <= 8e-2
        assert rel(smp(params[fx["gan/probe_names"][0]].grad), fx["gan/both/probe0/sample"]) <= 8e-2
        # (d) DMD2's generator GAN loss as it is written (dmd2.py:137-146): the full forward returns prediction AND taps, the
        # prediction is detached, only the taps carry gradient -> the same gradients as after the early return, and the decoder
        # is not differentiated at all
        net.zero_grad(set_to_none=True)
        xg = x0.clone().to(dev()).requires_grad_(True)
        o, fe = net(xg, t, condition=cond, feature_indices={0, 1, 2}, fwd_pred_type="x0")
        torch.autograd.backward(fe, dfs)
        assert rel(xg.grad, fx["gan/dx_early"]) <= 8e-2, rel(xg.grad, fx["gan/dx_early"])
        for n in fx["gan/probe_names"]:
            assert rel(smp(params[n].grad), fx[f"gan/early/{n}/sample"]) <= 8e-2, n
        g = params["model.dec.8x8_in0.conv0.weight"].grad
        assert g is None or float(g.abs().max()) == 0.0
    finally:
        net.requires_grad_(True)
        net.zero_grad(set_to_none=True)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_meanflow_network_backward_against_reference_golden(mf_nets, golden_dir, mode):
    """Autograd through the MeanFlow network (r_timestep embedding, drop_precond='both', unconditional, flow prediction): every
    parameter gradient and the input gradient against the reference's autograd (tests/golden/meanflow_backward_b2.pt).
    bf16x3 (the module's arithmetic without autocast = the reference's fp32 training precision for this config): relative L2 of the
    sampled entries <= 1e-3 for EVERY tensor, norms within 1e-3.  bf16: <= 1e-1 for every tensor, <= 6e-2 for 95 % of them, median
    <= 4e-2; norms within 3 %."""
    fx = load(golden_dir, "meanflow_backward_b2.pt")
    net = mf_nets[mode]
    x3 = mode == "bf16x3"
    params = dict(net.named_parameters())
    x = seeded((2, 3, 32, 32), 61).to(dev()).requires_grad_(True)
    dout = seeded((2, 3, 32, 32), 62).to(dev())
    try:
        net.zero_grad(set_to_none=True)
        out = net(x, fx["t"].to(dev()), r=fx["r"].to(dev()))
        check(out, fx["out"], mode, "MeanFlow forward under autograd")
        out.backward(dout)
        assert float((x.grad.cpu() - fx["dx"]).norm() / fx["dx"].norm()) <= (1e-3 if x3 else 8e-2)
        assert len(fx["names"]) > 400
        errs = []
        for n in fx["names"]:
            g = params[n].grad.detach().cpu().reshape(-1)
            smp = g[:: max(1, g.numel() // 512)][:512]
            want = fx[f"{n}/sample"]
            errs.append((float((smp - want).norm() / want.norm().clamp_min(1e-20)), n))
            assert abs(float(g.double().norm()) / float(fx[f"{n}/norm"]) - 1) <= (1e-3 if x3 else 3e-2), n
        errs.sort(reverse=True)
        print(mode, "worst five:", errs[:5], "median:", errs[len(errs) // 2][0])
        if x3:
            assert errs[0][0] <= 1e-3, errs[:5]
        else:
            # Accumulated bf16 rounding: every block's backward stores ~6 gradient tensors in bf16 (2^-9 relative each), so after 36
            # blocks the gradient signal carries sqrt(6 * 36) * 2^-9 ~ 3 % of independent noise - what bf16 autocast training has on
            # any backend; largest where few pixels are summed (8x8 layers at B = 2).  Every tensor <= 1e-1, 95 % <= 6e-2, median
            # <= 4e-2; the norms (above) within 3 %.  The per-block tests bound each block at 2e-2.
            assert errs[0][0] <= 1e-1, errs[:5]
            assert errs[len(errs) // 20][0] <= 6e-2, errs[: len(errs) // 20 + 1]
            assert errs[len(errs) // 2][0] <= 4e-2
    finally:
        net.zero_grad(set_to_none=True)


def test_module_under_distributed_data_parallel(nets, golden_dir):
    """The reference trains with DDP (trainer.ddp=True, fastgen/utils/distributed/ddp.py): the drop-in module must survive the
    wrapper - parameters registered, gradient hooks fired for every parameter the forward reads, the others (map_augment without
    augmentation labels, logvar_linear) reported unused exactly as the reference module reports them (it is wrapped with
    find_unused_parameters=True, configs/config.py:158-161, ddp.py:44-52); gradients identical to the bare module.  One rank
    here; two ranks: tests/test_gpu_dist.py."""
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP

    fx = load(golden_dir, "full_backward_b2.pt")
    net = nets["bf16"]
    t, cond = fx["t"].to(dev()), fx["cond"].to(dev())
    x = (seeded((2, 3, 32, 32), 21) * fx["t"].reshape(2, 1, 1, 1).float()).to(dev())
    dout = seeded((2, 3, 32, 32), 401).to(dev())
    created = False
    if not dist.is_initialized():
        import socket

        with socket.socket() as sk:  # a free port: nothing else on the box may hold a fixed one
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
        created = True
    try:
        net.zero_grad(set_to_none=True)
        (net(x, t, condition=cond, fwd_pred_type="x0") * dout).sum().backward()
        bare = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        net.zero_grad(set_to_none=True)
        ddp = DDP(net, device_ids=[0], find_unused_parameters=True)
        (ddp(x, t, condition=cond, fwd_pred_type="x0") * dout).sum().backward()
        got = {n: p.grad for n, p in net.named_parameters()}
        unused = {n for n, g in got.items() if g is None}
        assert unused == {"model.map_augment.weight", "model.logvar_linear.weight", "model.logvar_linear.bias"}, unused
        assert set(bare) == set(got) - unused
        for n, g in bare.items():
            assert torch.equal(got[n], g), n
    finally:
        net.zero_grad(set_to_none=True)
        if created:
            dist.destroy_process_group()


def test_network_backward_is_additive_over_the_batch(nets, sd):
    """Size-independent property, odd and single-image batches: every sample's contribution to the parameter gradients is
    independent of what else is in the batch (GroupNorm and attention are per image), so the gradients of a batch of 3 equal
    the sum of three batch-1 runs up to fp32 summation order and the bf16 rounding of differently-grouped partial sums."""
    g = torch.Generator().manual_seed(77)
    t = torch.tensor([3.1, 0.4, 41.0], dtype=torch.float64)
    x = torch.randn((3, 3, 32, 32), generator=g) * t.reshape(3, 1, 1, 1).float()
    cond = torch.nn.functional.one_hot(torch.tensor([1, 4, 9]), 10).float()
    dout = torch.randn((3, 3, 32, 32), generator=g)
    out3, g3 = _net_backward(nets["bf16"], sd, x, t, cond, dout)
    acc = None
    for i in range(3):
        o1, g1 = _net_backward(nets["bf16"], sd, x[i:i + 1], t[i:i + 1], cond[i:i + 1], dout[i:i + 1])
        assert torch.equal(o1[0], out3[i])  # the forward is bit-identical per sample
        acc = g1 if acc is None else {k: acc[k] + v for k, v in g1.items()}
    worst = max((float((g3[k] - acc[k]).norm() / acc[k].norm().clamp_min(1e-20)), k) for k in acc if float(acc[k].abs().max()) > 0)
    assert worst[0] <= 2e-3, worst


# ---- Discriminator_EDM heads --------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,idx", [("default", None), ("all", {0, 1, 2})])
def test_discriminator_edm_against_reference_golden(golden_dir, tag, idx):
    """Logits, feature-map gradients and every parameter gradient of the HIP Discriminator_EDM against the values recorded from
    the reference module under autograd (tests/golden/discriminator_edm.pt) and against the oracle's autograd in full:
    bf16 activations -> relative L2 <= 2e-2; logits to 3e-2 of their spread."""
    from tests.test_oracle_golden import _seeded_discriminator

    fx = load(golden_dir, "discriminator_edm.pt")
    d = _seeded_discriminator(idx).to(dev())
    bs = int(fx[f"{tag}/bs"])
    feats_cpu = [seeded((bs, 256, r, r), 510 + r) for r in d.in_res]
    dl = seeded(tuple(fx[f"{tag}/logits"].shape), 520)
    # oracle in full
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in d.state_dict().items()}
    fo = [f.clone().requires_grad_(True) for f in feats_cpu]
    with torch.enable_grad():
        R.discriminator_edm(sd, fo, d.in_res).backward(dl)
    # HIP
    feats = [f.to(dev()).requires_grad_(True) for f in feats_cpu]
    logits = d(feats)
    assert logits.shape == (bs, len(d.in_res))
    want = fx[f"{tag}/logits"]
    assert float((logits.detach().cpu() - want).abs().max()) <= 3e-2 * float(want.std() + want.abs().mean())
    logits.backward(dl.to(dev()))
    for f, o in zip(feats, fo):
        assert float((f.grad.cpu() - o.grad).norm() / o.grad.norm()) <= 2e-2
    for k, p in d.named_parameters():
        rel = float((p.grad.cpu() - sd[k].grad).norm() / sd[k].grad.norm().clamp_min(1e-20))
        assert rel <= 2e-2, (k, rel)
        assert abs(float(p.grad.double().norm()) / float(fx[f"{tag}/{k}/norm"]) - 1) <= 2e-2, k
    # forward only, no graph; CPU tensors are refused
    with torch.no_grad():
        again = d([f.detach() for f in feats])
    assert torch.equal(again, logits.detach())
    with pytest.raises(RuntimeError):
        d([f.detach().cpu() for f in feats])
    with pytest.raises(ValueError):
        d([feats[0].detach()] * (len(d.in_res) + 1))


def test_backward_sees_updated_weights(sd):
    """An optimizer step changes the parameters in place: the next forward / backward must use the new values everywhere,
    including the cached data-gradient weights and the transposed affine matrix (both rebuilt per weight version).  Checked
    against a fresh module that was constructed with the updated values."""
    def build(state):
        n = EDMPrecond(compute_dtype="bf16", **KW)
        n.load_state_dict(state, strict=True)
        return n.to(dev()).eval()

    g = torch.Generator().manual_seed(5)
    t = torch.tensor([1.3, 22.0], dtype=torch.float64, device=dev())
    x = (torch.randn((2, 3, 32, 32), generator=g) * 5).to(dev())
    cond = torch.nn.functional.one_hot(torch.tensor([2, 8]), 10).float().to(dev())
    dout = torch.randn((2, 3, 32, 32), generator=g).to(dev())
    probe = ["model.enc.32x32_block1.conv0.weight", "model.dec.16x16_block2.affine.weight", "model.enc.32x32_conv.weight",
             "model.dec.32x32_block2.skip.weight"]
    net = build(sd)
    (net(x, t, condition=cond) * dout).sum().backward()   # builds every cache with the old weights
    before = {k: dict(net.named_parameters())[k].grad.clone() for k in probe}
    with torch.no_grad():  # "optimizer step": every parameter moves
        gg = torch.Generator().manual_seed(6)
        for _, p in net.named_parameters():
            p.add_(0.05 * p.abs().mean() * torch.randn(p.shape, generator=gg).to(dev()))
    net.zero_grad(set_to_none=True)
    (net(x, t, condition=cond) * dout).sum().backward()
    fresh = build({k: v.detach().cpu() for k, v in net.state_dict().items()})
    (fresh(x, t, condition=cond) * dout).sum().backward()
    pf = dict(fresh.named_parameters())
    for k in probe:
        got, want = dict(net.named_parameters())[k].grad, pf[k].grad
        assert torch.equal(got, want), k                      # same kernels, same inputs: bit-identical
        assert not torch.equal(got, before[k]), k             # and the update was seen


# ---- forward mode ---------------------------------------------------------------------------------------------
def test_network_jvp_against_reference_func_jvp(nets, mf_nets, golden_dir):
    """fg_edm_jvp against `torch.func.jvp` through the reference (tests/golden/jvp_b2.pt): the MeanFlow network with the tangents
    MeanFlowModel._jvp uses, (dx/dt, 1, 0), and the preconditioned network with tangents in x_t and t.  bf16 compute:
    relative L2 <= 3e-2 on the derivative, the forward value to the forward tolerance."""
    fx = load(golden_dir, "jvp_b2.pt")
    v = seeded((2, 3, 32, 32), 72).to(dev())
    x = seeded((2, 3, 32, 32), 71).to(dev())
    t, r = fx["mf/t"].to(dev()), fx["mf/r"].to(dev())
    out, jv = mf_nets["bf16"].jvp(x, t, v, torch.ones_like(t), r=r, v_r=torch.zeros_like(r))
    check(out, fx["mf/out"], "bf16", "MeanFlow jvp primal")
    rel = float((jv.cpu() - fx["mf/jvp"]).norm() / fx["mf/jvp"].norm())
    assert rel <= 3e-2, rel
    from fastgen_amd.methods.consistency_model.mean_flow import MeanFlowModel as MF
    assert torch.equal(MF.network_jvp(mf_nets["bf16"], x, t, r, v), jv)  # the trainer-side helper: tangents (dx/dt, 1, 0)
    t = fx["edm/t"]
    x = (seeded((2, 3, 32, 32), 21) * t.reshape(2, 1, 1, 1)).to(dev())
    out, jv = nets["bf16"].jvp(x, t.to(dev()), v, fx["edm/vt"].to(dev()), condition=fx["edm/cond"].to(dev()))
    check(out, fx["edm/out"], "bf16", "EDM jvp primal")
    rel = float((jv.cpu() - fx["edm/jvp"]).norm() / fx["edm/jvp"].norm())
    assert rel <= 3e-2, rel
    # near the data end (c_out -> 0)
    t = fx["edm_small/t"]
    xs = (seeded((2, 3, 32, 32), 73) * 0.5).to(dev())
    out, jv = nets["bf16"].jvp(xs, t.to(dev()), v, fx["edm_small/vt"].to(dev()), condition=fx["edm/cond"].to(dev()))
    check(out, fx["edm_small/out"], "bf16", "EDM jvp primal, small t")
    rel = float((jv.cpu() - fx["edm_small/jvp"]).norm() / fx["edm_small/jvp"].norm())
    assert rel <= 3e-2, rel
    with pytest.raises(NotImplementedError):
        nets["fp32"].jvp(x, t.to(dev()), v)


def test_trigflow_wrapper_jvp_on_the_hip_network(nets, golden_dir):
    """sCM-family interface: TrigFlowPrecond around the HIP denoiser - forward and the composed forward-mode derivative against
    `torch.func.jvp` through the reference's wrapper (tests/golden/trigflow_b2.pt); bf16 compute, relative L2 <= 3e-2."""
    from fastgen_amd.methods.consistency_model.sCM import TrigFlowPrecond

    fx = load(golden_dir, "trigflow_b2.pt")
    w = TrigFlowPrecond(nets["bf16"], sigma_data=0.5)
    xh = (seeded((2, 3, 32, 32), 84) * 0.5).to(dev())
    vx = seeded((2, 3, 32, 32), 85).to(dev())
    t_hat, vt, cond = fx["wrap/t_hat"].to(dev()), fx["wrap/vt"].to(dev()), fx["wrap/cond"].to(dev())
    with torch.no_grad():
        F = w(xh, t_hat, condition=cond)
    assert float((F.cpu() - fx["wrap/F"]).norm() / fx["wrap/F"].norm()) <= 1e-2
    F2, dF = w.jvp(xh, t_hat, vx, vt, condition=cond)
    assert float((F2.cpu() - fx["wrap/F"]).norm() / fx["wrap/F"].norm()) <= 1e-2
    rel = float((dF.cpu() - fx["wrap/dF"]).norm() / fx["wrap/dF"].norm())
    assert rel <= 3e-2, rel


def test_network_jvp_properties_at_training_batch(nets):
    """Size-independent properties of the forward-mode pass at a training batch (B = 64): zero tangents give exactly zero (no
    stray additive term: biases and the label embedding carry no tangent), the derivative is linear in the tangents, the primal
    it returns is the ordinary forward, and a finite difference of the forward agrees with it in direction."""
    net = nets["bf16"]
    B = 64
    g = torch.Generator().manual_seed(3)
    t = (torch.rand(B, generator=g, dtype=torch.float64) * 20 + 0.5).to(dev())
    x = (torch.randn((B, 3, 32, 32), generator=g)).to(dev()) * t.reshape(B, 1, 1, 1).float()
    cond = torch.nn.functional.one_hot(torch.arange(B) % 10, 10).float().to(dev())
    vx = torch.randn((B, 3, 32, 32), generator=g).to(dev())
    vt = torch.randn(B, generator=g).to(dev()) * 0.1
    out0, z = net.jvp(x, t, torch.zeros_like(vx), torch.zeros_like(vt), condition=cond)
    assert float(z.abs().max()) == 0.0
    with torch.no_grad():
        assert torch.equal(out0, net(x, t, condition=cond))
    _, j1 = net.jvp(x, t, vx, vt, condition=cond)
    _, j2 = net.jvp(x, t, 2 * vx, 2 * vt, condition=cond)
    assert float((j2 - 2 * j1).norm() / (2 * j1).norm()) <= 1e-2   # exact up to bf16 rounding of the scaled tangents
    _, jx = net.jvp(x, t, vx, torch.zeros_like(vt), condition=cond)
    _, jt = net.jvp(x, t, torch.zeros_like(vx), vt, condition=cond)
    assert float((jx + jt - j1).norm() / j1.norm()) <= 2e-2
    # central finite difference of the fp32-mode forward (coarse: checks direction and scale, not digits)
    e = 1e-2
    with torch.no_grad():
        f = nets["fp32"]
        fd = (f(x + e * vx, t + e * vt.double(), condition=cond) - f(x - e * vx, t - e * vt.double(), condition=cond)) / (2 * e)
    cos = float((fd * j1).sum() / (fd.norm() * j1.norm()))
    assert cos >= 0.99 and abs(float(fd.norm() / j1.norm()) - 1) <= 5e-2, (cos, float(fd.norm() / j1.norm()))


def test_augmentation_labels(nets, golden_dir):
    """condition = {"aug_condition", "orig_condition"} (the training-time augmentation pipeline, EDM/network.py:903-915): forward in
    both compute modes and autograd (map_augment's gradient) against the reference (tests/golden/augment_b2.pt); a width that
    does not match map_augment is ignored like the reference does."""
    fx = load(golden_dir, "augment_b2.pt")
    t, cond = fx["t"].to(dev()), fx["cond"].to(dev())
    x = (seeded((2, 3, 32, 32), 91) * fx["t"].reshape(2, 1, 1, 1).float()).to(dev())
    aug = seeded((2, 9), 92).to(dev())
    dout = seeded((2, 3, 32, 32), 93).to(dev())
    c = {"aug_condition": aug, "orig_condition": cond}
    with torch.no_grad():
        for mode in ("fp32", "bf16"):
            check(nets[mode](x, t, condition=c, fwd_pred_type="x0"), fx["out"], mode, f"augment forward {mode}")
        plain = nets["fp32"](x, t, condition=cond, fwd_pred_type="x0")
        assert torch.equal(nets["fp32"](x, t, condition={"aug_condition": aug[:, :5], "orig_condition": cond}, fwd_pred_type="x0"), plain)
        assert torch.equal(nets["fp32"](x, t, condition=cond, fwd_pred_type="x0"), plain)  # the labels do not stick to the handle
    net = nets["bf16"]
    params = dict(net.named_parameters())
    try:
        net.zero_grad(set_to_none=True)
        (net(x, t, condition=c, fwd_pred_type="x0") * dout).sum().backward()
        g = params["model.map_augment.weight"].grad.cpu()
        assert float((g - fx["map_augment_grad"]).norm() / fx["map_augment_grad"].norm()) <= 5e-2
        for n in ("model.map_layer0.weight", "model.dec.32x32_block2.conv1.weight"):
            gg = params[n].grad.detach().cpu().reshape(-1)
            smp = gg[:: max(1, gg.numel() // 512)][:512]
            assert float((smp - fx[f"{n}/sample"]).norm() / fx[f"{n}/sample"].norm()) <= 8e-2, n
    finally:
        net.zero_grad(set_to_none=True)


def test_training_mode_dropout(sd, golden_dir):
    """dropout > 0 in train() mode (the SFT config's 0.13): the module draws a seed, the engine derives every block's mask from it
    (Philox) in the forward, the backward and the forward-mode pass.  The masks are read back with fg_op_dropout_mask and handed
    to the oracle, whose forward / autograd the HIP results must match (bf16 tolerances); eval mode and p = 0 are untouched."""
    L = _lib.lib()
    p = 0.13
    net = EDMPrecond(compute_dtype="bf16", **{**KW, "dropout": p})
    net.load_state_dict(sd, strict=True)
    net = net.to(dev())
    g = torch.Generator().manual_seed(11)
    t = torch.tensor([2.2, 0.31], dtype=torch.float64)
    x = torch.randn((2, 3, 32, 32), generator=g) * t.reshape(2, 1, 1, 1).float()
    cond = torch.nn.functional.one_hot(torch.tensor([0, 5]), 10).float()
    dout = torch.randn((2, 3, 32, 32), generator=g)
    net.eval()
    with torch.no_grad():
        ev = net(x.to(dev()), t.to(dev()), condition=cond.to(dev()))
    net.train()
    torch.manual_seed(77)
    seed = int(torch.randint(0, 2**62, (1,)).item())   # what the module will draw
    torch.manual_seed(77)
    out = net(x.to(dev()), t.to(dev()), condition=cond.to(dev()), fwd_pred_type="x0")
    (out * dout.to(dev())).sum().backward()
    assert not torch.allclose(out.detach(), ev, atol=1e-3)  # the dropout was applied
    # the masks the engine used, block by block (NHWC flat -> NCHW)
    enc, dec = R.layout(R.CIFAR10)
    blocks = [b for b in enc + dec if b.kind == "block"]
    keeps = {}
    for i, b in enumerate(blocks):
        m = torch.empty(2 * b.res * b.res * b.cout, device=dev())
        _lib.check(L.fg_op_dropout_mask(m.data_ptr(), m.numel(), p, i, seed, None))
        keeps[b.key] = m.reshape(2, b.res, b.res, b.cout).permute(0, 3, 1, 2).contiguous().cpu()
    frac = float(torch.cat([k.reshape(-1) for k in keeps.values()]).eq(0).float().mean())
    assert abs(frac - p) < 2e-3, frac                          # drop rate, and the survivors are scaled by 1 / (1 - p)
    assert float(keeps[blocks[0].key].max()) == pytest.approx(1 / (1 - p), rel=1e-6)
    names = ["model.enc.32x32_block1.conv1.weight", "model.enc.16x16_block2.norm1.weight", "model.dec.8x8_block1.conv0.weight"]
    sdg = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    with torch.enable_grad():
        want = R.edm_precond_forward(sdg, R.CIFAR10, x, t, cond, drop_keeps=keeps)
        want.backward(dout)
    check(out, want, "bf16", "training-mode forward with dropout")
    params = dict(net.named_parameters())
    for n in names:
        rel = float((params[n].grad.cpu() - sdg[n].grad).norm() / sdg[n].grad.norm())
        assert rel <= 8e-2, (n, rel)
    # the forward-mode pass sees the same masks: directional derivative along x against a finite difference of the oracle
    torch.manual_seed(77)
    v = torch.randn((2, 3, 32, 32), generator=g)
    _, jv = net.jvp(x.to(dev()), t.to(dev()), v.to(dev()), torch.zeros(2, device=dev()), condition=cond.to(dev()))
    e = 1e-2
    with torch.no_grad():
        fd = (R.edm_precond_forward(sd, R.CIFAR10, x + e * v, t, cond, drop_keeps=keeps)
              - R.edm_precond_forward(sd, R.CIFAR10, x - e * v, t, cond, drop_keeps=keeps)) / (2 * e)
    cos = float((fd * jv.cpu()).sum() / (fd.norm() * jv.cpu().norm()))
    assert cos >= 0.99, cos
