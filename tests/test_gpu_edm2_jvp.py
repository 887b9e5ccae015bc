"""EDM2Precond.jvp (fg_edm2_jvp) against torch.func.jvp of the fp64 restatement tests/edm2_ref.py: two networks, three tangents, sigma_shift
and every drop_precond, in both compute modes; the primal output bit-equal to forward(); zero / linear / additive tangents;
TrigFlowPrecond(EDM2Precond).jvp against torch.func.jvp through the same wrapper around the oracle; refusals and the workspace check.
tests/test_edm2_jvp_ref.py shows on the CPU that the thresholds pass the fp32 oracle and what they separate."""
import functools

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.methods.consistency_model.sCM import TrigFlowPrecond
from fastgen_amd.networks.noise_schedule import get_noise_schedule

import edm2_jvp_ref as J
import edm2_ops_ref as R
import edm2_ref as D
from test_gpu_edm2_ops import dev, make_net

pytestmark = pytest.mark.gpu

NETS = {"small_uncond": D.SMALL_UNCOND, "narrow": D.NARROW}
VARIANTS = {"base": {}, "shift": dict(sigma_shift=0.003), "drop_input": dict(drop_precond="input"), "drop_output": dict(drop_precond="output"),
            "drop_both": dict(drop_precond="both")}
B = 2


@functools.lru_cache(maxsize=None)
def oracle(name, variant):
    """Inputs and the fp64 oracle's (out, {tangent kind: jvp}) of one case, shared by the two compute modes.  The clamp stays open:
    every activation of the oracle is below 0.9 clip_act."""
    cfg = NETS[name]
    sd = D.random_state_dict(cfg, seed=1234)
    x, t, lab, vx, vt = J.net_inputs(cfg, B, 71)
    trace = {}
    ref = {}
    for k in ("x", "t"):
        out, ref[k] = J.precond_jvp(sd, cfg, x, t, lab, *J.tangent(k, vx, vt), trace=trace if k == "x" else None, **VARIANTS[variant])
    ref["both"] = ref["x"] + ref["t"]  # linear in the tangent
    assert max(v.abs().max().item() for k, v in trace.items() if k != "emb") < 0.9 * cfg.clip_act
    return sd, (x, t, lab, vx, vt), out, ref


def gpu(*ts):
    return [None if a is None else a.to(dev()) for a in ts]


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(NETS))
def test_jvp_against_fp64(name, variant, mode):
    """Worst per-image relative L2 and max |d| of the jvp against the fp64 oracle, thresholds J.NET_JVP_TOL.  Measured on an MI355X
    over the 10 cases x 3 tangents, worst: bf16x3 rel L2 1.77e-5 (small_uncond, drop_both, t), max_abs 6.9e-5 (narrow, drop_both,
    both); bf16 rel L2 8.7e-3, max_abs 4.1e-2 (the same two cases); the thresholds are 1.5x these.  The fp32 CPU oracle lies at rel
    3e-7.  tests/test_edm2_jvp_ref.py::test_net_jvp_mutants says, per image, which structural mutants each mode's thresholds
    separate: bf16x3 all of them (the closest at 4.7e-4, 17x), bf16 those of its table.  The primal is forward()'s, bit for bit."""
    cfg = NETS[name]
    sd, (x, t, lab, vx, vt), ref_out, ref = oracle(name, variant)
    net = make_net(cfg, sd, compute_dtype=mode, **VARIANTS[variant])
    dx, dt, dlab, dvx, dvt = gpu(x, t, lab, vx, vt)
    with torch.no_grad():
        fwd = net(dx, dt, condition=dlab)
    worst = [0.0, 0.0]
    for k in J.TANGENTS:
        a, b = J.tangent(k, dvx, dvt)
        out, jv = net.jvp(dx, dt, a, None if k == "x" else b, condition=dlab)
        assert torch.equal(out, fwd) and torch.isfinite(jv).all()
        rel, mx = J.per_image(jv.cpu(), ref[k])
        print(f"\nedm2 jvp {name} {variant} {mode} {k}: rel L2 {rel:.2e} max_abs {mx:.2e}")
        worst = [max(worst[0], rel), max(worst[1], mx)]
    tol = J.NET_JVP_TOL[mode]
    assert worst[0] <= tol["rel"] and worst[1] <= tol["max_abs"], (worst, tol)
    del net
    torch.cuda.empty_cache()


def test_jvp_properties():
    """At B = 8 on NARROW (bf16x3): zero tangents give exactly zero, the primal is the ordinary forward, the derivative is linear in
    the tangent and additive over (v_x, v_t) to rounding (1e-4: five times the per-block bound 2e-5), and v_t = None is v_t = 0."""
    cfg = D.NARROW
    net = make_net(cfg, D.random_state_dict(cfg, seed=1234), compute_dtype="bf16x3")
    x, t, lab, vx, vt = gpu(*J.net_inputs(cfg, 8, 73))
    out0, z = net.jvp(x, t, torch.zeros_like(vx), torch.zeros_like(vt), condition=lab)
    assert float(z.abs().max()) == 0.0
    with torch.no_grad():
        assert torch.equal(out0, net(x, t, condition=lab))
    _, j1 = net.jvp(x, t, vx, vt, condition=lab)
    _, j2 = net.jvp(x, t, 1.7 * vx, 1.7 * vt, condition=lab)
    assert float((j2 - 1.7 * j1).norm() / (1.7 * j1).norm()) <= 1e-4
    _, jx = net.jvp(x, t, vx, torch.zeros_like(vt), condition=lab)
    _, jt = net.jvp(x, t, torch.zeros_like(vx), vt, condition=lab)
    assert float((jx + jt - j1).norm() / j1.norm()) <= 1e-4
    assert torch.equal(net.jvp(x, t, vx, condition=lab)[1], jx)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_trigflow_jvp(mode):
    """TrigFlowPrecond(EDM2Precond).jvp - sCM's call - against torch.func.jvp through the same wrapper around the fp64 oracle, under the
    whole-network thresholds.  Measured on an MI355X: bf16x3 rel L2 1.1e-5, bf16 6.1e-3."""
    cfg = D.NARROW
    sd = D.random_state_dict(cfg, seed=1234)
    sd64 = R.to64(sd)

    class OracleNet(torch.nn.Module):
        noise_scheduler = get_noise_schedule("edm")

        def forward(self, x, t, condition=None, return_logvar=False, fwd_pred_type="x0"):
            return D.precond_forward(sd64, cfg, x, t, condition)

    g = R.gen(75)
    xh = torch.randn(B, 3, 64, 64, generator=g) * 0.5
    vx = torch.randn(B, 3, 64, 64, generator=g)
    th, vt = torch.tensor([0.6, 1.2]), torch.tensor([0.9, -0.4])
    lab = torch.nn.functional.one_hot(torch.arange(B) * 3 % cfg.label_dim, cfg.label_dim).float()
    w64 = TrigFlowPrecond(OracleNet(), sigma_data=cfg.sigma_data)
    ref, ref_d = torch.func.jvp(lambda a, b: w64(a, b, condition=lab.double()), (xh.double(), th.double()), (vx.double(), vt.double()))
    w = TrigFlowPrecond(make_net(cfg, sd, compute_dtype=mode), sigma_data=cfg.sigma_data)
    F, dF = w.jvp(*gpu(xh, th, vx, vt), condition=lab.to(dev()))
    (rel0, _), (rel, _) = J.per_image(F.cpu(), ref), J.per_image(dF.cpu(), ref_d)
    print(f"\ntrigflow jvp {mode}: F rel L2 {rel0:.2e}, dF rel L2 {rel:.2e}")
    assert rel0 <= J.NET_JVP_TOL[mode]["rel"] and rel <= J.NET_JVP_TOL[mode]["rel"], (rel0, rel)


def test_refusals_and_workspace():
    cfg = D.SMALL_UNCOND
    net = make_net(cfg, D.random_state_dict(cfg, seed=1234), compute_dtype="bf16x3")
    x, t, lab, vx, vt = gpu(*J.net_inputs(cfg, B, 71))
    with pytest.raises(ValueError):
        net.jvp(x, t, vx, vt, r=t)
    with pytest.raises(NotImplementedError):
        net.jvp(x, t, vx, vt, fwd_pred_type="eps")
    drop = make_net(cfg, D.random_state_dict(cfg, seed=1234), compute_dtype="bf16x3", dropout=0.1).train()
    with pytest.raises(NotImplementedError):
        drop.jvp(x, t, vx, vt)
    # a workspace one byte short is refused (FG_EINVAL = 1) before anything is launched: out / jvp keep their fill
    L = _lib.lib()
    dt, h = net._engine(dev())
    need = L.fg_edm2_jvp_workspace_bytes(h, B)
    assert need > L.fg_edm2_workspace_bytes(h, B)
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    out, jv = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    args = lambda n: (h, x.data_ptr(), t.data_ptr(), None, vx.data_ptr(), vt.data_ptr(), out.data_ptr(), jv.data_ptr(), B, ws.data_ptr(), n, None)  # noqa: E731
    assert L.fg_edm2_jvp(*args(need - 1)) == 1
    torch.cuda.synchronize()
    assert (out == 7).all() and (jv == 7).all()
    assert L.fg_edm2_jvp(*args(need)) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(jv).all() and torch.equal(jv, net.jvp(x, t, vx, vt)[1])
