"""`DiT.jvp` / `fg_dit_jvp` (fastgen_amd/csrc/engine_dit.inc `dit_jvp`, kernels dit_jvp.hip + the split-bf16 token GEMM) against
`torch.func.jvp` over the oracle's `dit_forward` in fp64 (oracle/dit_ref.py; what MeanFlowModel._jvp evaluates, mean_flow.py:240-250).

Networks: `random_state_dict(cfg, seed=77)`, depth 2, S width (384, 6 heads of 64) at B = 3 and B = 9, XL width (1152, 16 heads of 72)
at B = 3; configurations: r_timestep with time_cond_type "diff" and scale_t off (the reference's MeanFlow-XL config), r_timestep "abs"
with scale_t on, no r with the SiT convention.  Three tangent directions are checked separately - (v_x, 0, 0), (0, 1, 0) and
(v_x, 1, v_r != 0): under scale_t the time direction is two orders of magnitude larger than the x direction, and a combined check alone
would hide a wrong x path.  The granule is one sample's output (every sample has its own x, t, r, class and tangent).

Bounds (relative L2, max |err| / max |ref|) per sample, twice the worst measured on an MI355X over that matrix:
    tangent, x direction                        5.02e-6 / 5.53e-6  (XL abs-scale_t B 3 / S abs-scale_t B 3)
    tangent, a direction with v_t, scale_t off  7.22e-6 / 7.63e-6  (XL diff B 3, (0, 1, 0))
    tangent, a direction with v_t, scale_t on   2.04e-5 / 2.21e-5  (S abs-scale_t B 9, (v_x, 1, v_r))
    out against the oracle                      5.48e-6 / 6.82e-6  (S abs-scale_t B 9 / XL abs-scale_t B 3)
The time direction under scale_t has a bound of its own: the embedder sees t_e = 1000 t in fp32, half an ulp of which (3e-5 at
t_e = 500) is an absolute error of the fastest Fourier angle, and the time tangent is carried by exactly those features - the
reference's own float32 evaluation (precision_amp_jvp) has the same.  `out` against `forward()` on the same inputs: relative L2
<= 2.5e-5, the bf16x3 increment bound of tests/test_gpu_dit_blocks.py (worst measured 1.92e-6).  Discrimination: test_mutants - the
closest mutant, the oracle with bf16-rounded block weights, misses its bound 35 times over (sit, time direction); every other one by more than 2000 times."""
import pytest
import torch

import dit_jvp_ref as J
from oracle import dit_ref as R

pytestmark = pytest.mark.gpu

WIDTH = {"S": dict(hidden_size=384, num_heads=6), "XL": dict(hidden_size=1152, num_heads=16)}
CONFIG = {
    "diff": dict(r_timestep=True, time_cond_type="diff", scale_t=False),
    "abs-scale_t": dict(r_timestep=True, time_cond_type="abs", scale_t=True),
    "sit": dict(use_sit_convention=True),
}
CASES = [(w, c, b) for w, b in (("S", 3), ("XL", 3), ("S", 9)) for c in CONFIG]
DIRECTIONS = ("x", "t", "xtr")
# (relative L2, max |err| / max |ref|) per sample: 2 x the worst measured (module docstring)
TOL = {"x": (1.0e-5, 1.1e-5), "t": (1.5e-5, 1.6e-5), "t-scaled": (4.1e-5, 4.5e-5), "out": (1.1e-5, 1.4e-5)}
TOL_FWD = 2.5e-5
F64 = torch.float64
_NET, _RES = {}, {}


def _net(width, config):
    key = (width, config)
    if key not in _NET:
        from fastgen_amd.networks.DiT.network import DiT

        kw = dict(depth=2, **WIDTH[width], **CONFIG[config])
        cfg = R.DiTConfig(**kw)
        sd = R.random_state_dict(cfg, seed=77)
        net = DiT(compute_dtype="bf16x3", **kw)
        net.load_state_dict(sd, strict=True)
        _NET.clear()  # one network's engine at a time
        _NET[key] = (net.to("cuda:0").eval(), cfg, {k: v.double() for k, v in sd.items()})
    return _NET[key]


def _inputs(cfg, B):
    """x, t, r < t, class (sample 1: the unconditional row) and tangents v_x, v_r of its own per sample."""
    g = torch.Generator().manual_seed(31 * B + cfg.hidden_size)
    x, vx = (torch.randn(B, 4, 32, 32, generator=g, dtype=F64) for _ in range(2))
    t = 0.05 + 0.9 * torch.rand(B, generator=g, dtype=F64)
    r = t * torch.rand(B, generator=g, dtype=F64) if cfg.r_timestep else None
    vr = torch.randn(B, generator=g, dtype=F64) if cfg.r_timestep else None
    cls = torch.randperm(1000, generator=g)[:B]
    cls[1] = 1000
    return x, t, r, cls, vx, vr


def _tangents(direction, vx, vr, B):
    zx, one, zero = torch.zeros_like(vx), torch.ones(B, dtype=F64), torch.zeros(B, dtype=F64)
    has_r = vr is not None
    return {"x": (vx, zero, zero if has_r else None), "t": (zx, one, zero if has_r else None), "xtr": (vx, one, vr)}[direction]


def _gpu(net, x, t, r, cls, vx, vt, vr, rows=slice(None)):
    f = lambda a: None if a is None else a[rows].float().cuda()  # noqa: E731
    out, jv = net.jvp(f(x), f(t), f(vx), f(vt), condition=cls[rows].cuda(), r=f(r), v_r=f(vr))
    return out.double().cpu(), jv.double().cpu()


def _rows(B):
    return list(range(B)) if B <= 3 else [0, 1, B // 2, B - 1]


def _case(width, config, B):
    """GPU results and fp64 references of one case, all directions, computed once and shared (nothing changes them):
    {direction: (gpu out, gpu jvp, ref out, ref jvp)} on the checked rows, plus the inputs."""
    key = (width, config, B)
    if key not in _RES:
        net, cfg, sd = _net(width, config)
        x, t, r, cls, vx, vr = _inputs(cfg, B)
        rows = _rows(B)
        res = {}
        for d in DIRECTIONS:
            tx, tt, tr = _tangents(d, vx, vr, B)
            go, gj = _gpu(net, x, t, r, cls, tx, tt, tr)
            pick = lambda a: None if a is None else a[rows]  # noqa: E731
            ro, rj = J.oracle_jvp(sd, cfg, x[rows], t[rows], cls[rows], pick(r), tx[rows], tt[rows], pick(tr))
            res[d] = (go[rows], gj[rows], ro, rj)
        _RES[key] = (res, (x, t, r, cls, vx, vr))
    return _RES[key]


def _tol(direction, cfg):
    return TOL["x" if direction == "x" else "t-scaled" if cfg.scale_t else "t"]


def _err(got, ref):
    e = (got - ref).flatten(1)
    return (e.norm(dim=1) / ref.flatten(1).norm(dim=1)).max().item(), (e.abs().amax(1) / ref.flatten(1).abs().amax(1)).max().item()


@pytest.mark.parametrize("width,config,B", CASES, ids=[f"{w}-{c}-B{b}" for w, c, b in CASES])
def test_jvp_against_the_oracle(width, config, B):
    res, (x, t, r, cls, vx, vr) = _case(width, config, B)
    net, cfg, _ = _net(width, config)
    figs, bad = [], []
    for d in DIRECTIONS:
        go, gj, ro, rj = res[d]
        assert bool(torch.isfinite(go).all() and torch.isfinite(gj).all())
        ej, eo = _err(gj, rj), _err(go, ro)
        figs.append(f"{d}: jvp {ej[0]:.2e} / {ej[1]:.2e} (|ref| {rj.norm().item():.3g}) out {eo[0]:.2e} / {eo[1]:.2e}")
        bad += [(d, k, e) for k, e, b in (("jvp", ej, _tol(d, cfg)), ("out", eo, TOL["out"])) if not (e[0] <= b[0] and e[1] <= b[1])]
    # the primal output: what forward() returns on the same inputs, to the increment bound of the bf16x3 blocks; the same for every tangent
    f = lambda a: None if a is None else a.float().cuda()  # noqa: E731
    with torch.no_grad():
        fwd = net(f(x), f(t), condition=cls.cuda(), r=f(r)).double().cpu()[_rows(B)]
    efw = max(_err(res[d][0], fwd)[0] for d in DIRECTIONS)
    print(f"\n[dit-jvp] {width} {config} B {B}: " + "  ".join(figs) + f"  out against forward() {efw:.2e}")
    assert efw <= TOL_FWD, efw
    assert torch.equal(res["x"][0], res["t"][0]) and torch.equal(res["x"][0], res["xtr"][0])
    assert not bad, bad


@pytest.mark.parametrize("width,config", [("S", "diff"), ("XL", "abs-scale_t")])
def test_second_call_returns_the_same_bits(width, config):
    res, (x, t, r, cls, vx, vr) = _case(width, config, 3)
    net = _net(width, config)[0]
    go, gj = _gpu(net, x, t, r, cls, *_tangents("xtr", vx, vr, 3))
    assert torch.equal(go, res["xtr"][0]) and torch.equal(gj, res["xtr"][1])


def test_batch_rows_are_independent():
    """Rows 1:3 of the B = 9 call equal a B = 2 call on those rows."""
    for config in ("diff", "sit"):
        net, cfg, sd = _net("S", config)
        x, t, r, cls, vx, vr = _inputs(cfg, 9)
        tg = _tangents("xtr", vx, vr, 9)
        go9, gj9 = _gpu(net, x, t, r, cls, *tg)
        go2, gj2 = _gpu(net, x, t, r, cls, *tg, rows=slice(1, 3))
        assert torch.equal(go9[1:3], go2) and torch.equal(gj9[1:3], gj2), config


def test_meanflow_network_jvp():
    """MeanFlowModel.network_jvp(net, x_t, t, r, dxt_dt) is the (dxt_dt, 1, 0) tangent (mean_flow.py:240-250)."""
    from fastgen_amd.methods.consistency_model.mean_flow import MeanFlowModel

    net, cfg, sd = _net("S", "diff")
    x, t, r, cls, vx, vr = _inputs(cfg, 3)
    f = lambda a: a.float().cuda()  # noqa: E731
    got = MeanFlowModel.network_jvp(net, f(x), f(t), f(r), f(vx), condition=cls.cuda()).double().cpu()
    want = J.oracle_jvp(sd, cfg, x, t, cls, r, vx, torch.ones(3, dtype=F64), torch.zeros(3, dtype=F64))[1]
    e = _err(got, want)
    print(f"\n[dit-jvp] network_jvp: {e[0]:.2e} / {e[1]:.2e}")
    assert e[0] <= TOL["t"][0] and e[1] <= TOL["t"][1], e


def _far(mutant, ref, bound):
    """How many times the closest sample of a mutated reference misses the bound (the smaller of the two measures)."""
    e = (mutant - ref).flatten(1)
    rel = (e.norm(dim=1) / ref.flatten(1).norm(dim=1)).min().item() / bound[0]
    mx = (e.abs().amax(1) / ref.flatten(1).abs().amax(1)).min().item() / bound[1]
    return min(rel, mx)


@pytest.mark.parametrize("config", list(CONFIG))
def test_mutants(config):
    """The bound discriminates: references mutated in fp64 from the oracle alone each miss it by at least 5 times in every sample of
    the direction where they act, and so does the GPU result measured against them."""
    res, (x, t, r, cls, vx, vr) = _case("S", config, 3)
    net, cfg, sd = _net("S", config)
    B = 3
    mut = {}
    full = {d: J.dit_jvp(sd, cfg, x, t, cls, r, *_tangents(d, vx, vr, B))[1] for d in DIRECTIONS}
    for d in DIRECTIONS:  # (the mirror itself is the oracle: tests/test_dit_jvp_ref.py, here once more on these inputs)
        assert _err(full[d], res[d][3])[0] < 1e-10
    m = lambda d, **kw: J.dit_jvp(sd, cfg, x, t, cls, r, *_tangents(d, vx, vr, B), **kw)[1]  # noqa: E731
    mut["a: no softmax-derivative term / x"] = ("x", m("x", drop_softmax_term=True))
    mut["a: no softmax-derivative term / t"] = ("t", m("t", drop_softmax_term=True))
    mut["b: no gate-tangent terms / t"] = ("t", m("t", drop_gate_tangent=True))
    mut["b: no gate-tangent terms / xtr"] = ("xtr", m("xtr", drop_gate_tangent=True))
    mut["c: no n sd + bd terms / t"] = ("t", m("t", drop_mod_tangent=True))
    mut["c: no n sd + bd terms / xtr"] = ("xtr", m("xtr", drop_mod_tangent=True))
    mut["d: the neighbouring sample's tangent / x"] = ("x", res["x"][3].roll(1, 0))
    mut["d: the neighbouring sample's tangent / t"] = ("t", res["t"][3].roll(1, 0))
    if config == "diff":
        mut["e: v_r with the wrong sign / xtr"] = ("xtr", m("xtr", flip_vr=True))
    lin = ("attention.qkv.weight", "attention.proj.weight", "feed_forward.fc1.weight", "feed_forward.fc2.weight")
    sd16 = {k: (v.float().bfloat16().double() if k.startswith("blocks.") and k.endswith(lin) else v) for k, v in sd.items()}
    for d in ("x", "t"):
        mut[f"f: bf16-rounded block weights / {d}"] = (d, J.oracle_jvp(sd16, cfg, x, t, cls, r, *_tangents(d, vx, vr, B))[1])
    report, bad = [], []
    for name, (d, ref_m) in mut.items():
        far_ref, far_gpu = _far(ref_m, res[d][3], _tol(d, cfg)), _far(ref_m, res[d][1], _tol(d, cfg))
        report.append(f"{name}: {far_ref:.3g} x (GPU {far_gpu:.3g} x)")
        if not (far_ref >= 5 and far_gpu >= 5):
            bad.append((name, far_ref, far_gpu))
    print(f"\n[dit-jvp] mutants {config} (times the bound, closest sample): " + "; ".join(report))
    assert not bad, bad
