"""Wan2.2 TI2V-5B on the GPU: `WanI2V(concat_mask=False, use_image_encoder=False, expand_timesteps=True)` (fg_wan_create_ti2v,
fg_wan_set_first_frame and `Wan`'s entry points on that handle) and `Wan(expand_timesteps=True)` on the 2-block 48-channel network of
tests/wan_ti2v_ref.py, against that file's oracle (per-TOKEN timesteps, literal replacement) and away from its mutants, which
tests/test_wan_ti2v_ref.py holds at least 5 x TOL apart on the CPU.  PARITY UNPINNED like everything `fg_wan_*`.
TOL = 2e-2: this network's tolerance in tests/test_gpu_wan_full.py.  The fp8 band is tests/test_gpu_wan_fp8.py's: at most 2 E_Q from
the plain oracle and more than 0.25 E_Q from the bf16 mode, with the largest / smallest E_Q of tests/wan_fp8_ref.py."""
import ctypes
import socket

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks._engine import ptr
from oracle import wan_ref as R
import wan_fp8_ref as Q
import wan_ti2v_ref as T

pytestmark = pytest.mark.gpu

KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2)
TI2V = dict(concat_mask=False, use_image_encoder=False, expand_timesteps=True, image_dim=None, in_channels=48, out_channels=48)
TOL = 2e-2
E_Q_MAX, E_Q_MIN = max(max(v.values()) for v in Q.E_Q.values()), min(min(v.values()) for v in Q.E_Q.values())
FG_EINVAL = 1


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _net(sd, **kw):
    from fastgen_amd.networks.WanI2V.network import WanI2V

    net = WanI2V(**dict(dict(KW, **TI2V), **kw))
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


def _gpu_cond(cond):
    return {"text_embeds": cond["text"].cuda(), "first_frame_cond": cond["ff"].cuda()}


@pytest.fixture(scope="module")
def case():
    return T.case()


# ---- 1. forward: the two networks against the oracle --------------------------------------------------------------------------------
def test_i2v_forward_against_oracle_and_its_mutants(case):
    sd, x, t, cond = case
    net = _net(sd)
    gc = _gpu_cond(cond)
    with torch.inference_mode():
        flow = net(x.cuda(), t.cuda(), condition=gc).cpu()
        x0 = net(x.cuda(), t.cuda(), condition=gc, fwd_pred_type="x0").cpu()
        with pytest.raises(NotImplementedError, match=r"t must be \[B\]"):
            net(x.cuda(), torch.zeros(2, 480).cuda(), condition=gc)
    ref = T.WanTI2VRef(sd, T.TINY48)
    want = ref.forward(x, t, cond, fwd_pred_type="x0")
    d, d_flow = _rel(x0, want), _rel(flow, ref.forward(x, t, cond))
    print("ti2v forward vs oracle: x0", d, "flow", d_flow)
    assert torch.isfinite(x0).all() and torch.isfinite(flow).all() and d < TOL and d_flow < TOL, (d, d_flow)
    # frame 0 of the result is the condition's whatever the prediction type
    assert torch.equal(x0[:, :, 0], cond["ff"][:, :, 0]) and torch.equal(flow[:, :, 0], cond["ff"][:, :, 0])
    for m in T.MUTANTS:
        bad = T.WanTI2VRef(sd, T.TINY48, mutant=m).forward(x, t, cond, fwd_pred_type="x0")
        rest = m in T.INPUT_SIDE
        dm = _rel(x0[:, :, 1:], bad[:, :, 1:]) if rest else _rel(x0, bad)
        err = _rel(x0[:, :, 1:], want[:, :, 1:]) if rest else d
        print("  mutant", m, dm, "measured error", err)
        assert dm >= 5 * err, (m, dm, err)
    # a full-length condition: only frame 0 is read
    full = torch.cat([gc["first_frame_cond"], torch.full((2, 48, 4, 16, 24), 9.0, device="cuda")], dim=2)
    with torch.inference_mode():
        assert torch.equal(net(x.cuda(), t.cuda(), condition=dict(gc, first_frame_cond=full), fwd_pred_type="x0").cpu(), x0)


def test_t2v_forward_with_expanded_timesteps(case):
    from fastgen_amd.networks.Wan.network import Wan

    sd, x, t, cond = case
    nets = [Wan(**KW, in_channels=48, out_channels=48, expand_timesteps=e) for e in (True, False)]
    outs = []
    for n in nets:
        n.load_state_dict(sd, strict=True)
        with torch.inference_mode():
            outs.append(n.cuda().eval()(x.cuda(), t.cuda(), condition=cond["text"].cuda()).cpu())
    d = _rel(outs[0], T.WanTI2VRef(sd, T.TINY48, i2v=False).forward(x, t, cond))
    print("t2v (expand_timesteps) forward vs oracle", d)
    assert torch.isfinite(outs[0]).all() and d < TOL and torch.equal(outs[0], outs[1])
    # ... and it is not the image-to-video network
    assert _rel(outs[0], T.WanTI2VRef(sd, T.TINY48).forward(x, t, cond)) >= 5 * TOL


# ---- 2. the 5B network's width ------------------------------------------------------------------------------------------------------
def test_width_of_the_5b_network_against_oracle():
    cfg = R.WanConfig(num_heads=24, head_dim=128, in_channels=48, out_channels=48, text_dim=256, ffn_dim=14336, num_layers=1)
    sd = R.random_state_dict(cfg, 91)
    g = torch.Generator().manual_seed(92)
    x, t = torch.randn(1, 48, 2, 16, 16, generator=g), torch.tensor([0.7], dtype=torch.float64)
    cond = {"text": torch.randn(1, 9, 256, generator=g), "ff": torch.randn(1, 48, 1, 16, 16, generator=g)}
    kw = dict(num_attention_heads=24, text_dim=256, ffn_dim=14336, num_layers=1)
    want = T.WanTI2VRef(sd, cfg).forward(x, t, cond)
    out = {}
    for mode in ("bf16", "fp8"):
        net = _net(sd, compute_dtype=mode, **kw)
        with torch.inference_mode():
            out[mode] = net(x.cuda(), t.cuda(), condition=_gpu_cond(cond)).cpu()
        del net
    d16, d8, d816 = _rel(out["bf16"][:, :, 1:], want[:, :, 1:]), _rel(out["fp8"][:, :, 1:], want[:, :, 1:]), _rel(out["fp8"], out["bf16"])
    print("5B width vs oracle: bf16", d16, "fp8", d8, "fp8 vs bf16", d816)
    assert torch.isfinite(out["bf16"]).all() and d16 < TOL, d16
    assert torch.isfinite(out["fp8"]).all() and not torch.equal(out["fp8"], out["bf16"])
    assert d8 <= 2 * E_Q_MAX and _rel(out["fp8"][:, :, 1:], out["bf16"][:, :, 1:]) > 0.25 * E_Q_MIN, (d8, d816)


# ---- 3. the fused x0 loop -----------------------------------------------------------------------------------------------------------
def test_fused_x0_loop_equals_the_generic_loop_with_the_hook(monkeypatch, case):
    from fastgen_amd.methods.model import FastGenModel

    sd, x, _, cond = case
    net = _net(sd)
    gc = _gpu_cond(cond)
    g = torch.Generator().manual_seed(84)
    noise, eps = x.cuda(), torch.randn((1, *T.SHAPE), generator=g).cuda()
    sch = net.noise_scheduler
    TL = [0.999, 0.833, 0.0]

    def per_step(c, kind):
        """the generic loop: one forward per step, `preserve_conditioning` on every prediction and every re-noised state"""
        tl = torch.tensor(TL, dtype=sch.t_precision).cuda()
        pending = [e for e in eps]
        monkeypatch.setattr(torch, "randn_like", lambda x_, **kw: pending.pop(0))
        with torch.inference_mode():
            out = FastGenModel._student_sample_loop(net, sch.latents(noise, tl[0]), tl, condition=c, student_sample_type=kind)
        monkeypatch.undo()
        return out

    kw = dict(student_sample_steps=2, t_list=TL, eps=eps)
    want = {}
    for kind in ("sde", "ode"):
        want[kind] = per_step(gc, kind)
        got = FastGenModel.generator_fn(net, noise, student_sample_type=kind, condition=gc, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, want[kind]), kind
        assert torch.equal(got[:, :, 0], gc["first_frame_cond"][:, :, 0])
        assert torch.equal(FastGenModel.generator_fn(net, noise, student_sample_type=kind, condition=gc, use_graph=False, **kw), want[kind]), kind
    # new first-frame contents at the same shape: the cached graph, the new result
    gc2 = dict(gc, first_frame_cond=torch.randn(2, 48, 1, 16, 24, generator=g).cuda())
    captures, launches = _lib.graph_stats()
    got2 = FastGenModel.generator_fn(net, noise, student_sample_type="ode", condition=gc2, **kw)
    assert _lib.graph_stats() == (captures, launches + 1), "new contents at the same shape captured a new graph"
    assert torch.equal(got2, FastGenModel.generator_fn(net, noise, student_sample_type="ode", condition=gc2, use_graph=False, **kw))
    assert torch.equal(got2, per_step(gc2, "ode")) and not torch.equal(got2, want["ode"])
    # the handle's copy is the new condition
    back = torch.empty(2, 48, 1, 16, 24, device="cuda")
    _lib.check(_lib.lib().fg_wan_first_frame_read(net._h, ptr(back), None))
    torch.cuda.synchronize()
    assert torch.equal(back, gc2["first_frame_cond"])
    # ... and against the oracle's loop
    ref = T.WanTI2VRef(sd, T.TINY48)
    oracle = T.x0_loop(ref, x, torch.tensor(TL, dtype=torch.float64), cond, eps_list=[eps[0].cpu()], sample_type="sde")
    d = _rel(want["sde"].cpu(), oracle)
    print("ti2v fused x0 loop vs oracle", d)
    assert d < 2 * TOL, d  # (two network calls)


# ---- 4. sample() --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["unipc", "euler"])
def test_guided_sample(solver, case):
    G, STEPS, SHIFT = 1.5, 3, 3.0  # (tests/test_gpu_wan_i2v.py's case)
    sd, x, _, cond = case
    g = torch.Generator().manual_seed(86)
    neg = {"text": -cond["text"], "ff": torch.randn(2, 48, 1, 16, 24, generator=g)}
    net = _net(sd)
    gc, gn, noise = _gpu_cond(cond), _gpu_cond(neg), x.cuda()
    kw = dict(guidance_scale=G, num_steps=STEPS, solver=solver)
    with torch.inference_mode():
        got = net.sample(noise, gc, gn, **kw)
        assert torch.isfinite(got).all() and torch.equal(got[:, :, 0], gc["first_frame_cond"][:, :, 0])
        assert torch.equal(net.sample(noise, gc, gn, use_graph=False, **kw), got)
        swapped = net.sample(noise, dict(gc, first_frame_cond=gn["first_frame_cond"]), dict(gn, first_frame_cond=gc["first_frame_cond"]), **kw)
        unguided = net.sample(noise, gc, None, guidance_scale=None, num_steps=STEPS, solver=solver)
        assert torch.equal(unguided[:, :, 0], gc["first_frame_cond"][:, :, 0])
    ref = T.WanTI2VRef(sd, T.TINY48, dtype=torch.float64)
    oracle = T.guided_sample(ref, x.double(), cond, neg, G, STEPS, shift=SHIFT, solver=solver)
    d, dsw = _rel(got.cpu(), oracle), _rel(swapped.cpu(), oracle)
    print("ti2v guided sample vs oracle", solver, d, "first frames swapped", dsw)
    assert d < TOL and dsw > d, (d, dsw)
    d1 = _rel(unguided.cpu(), T.guided_sample(ref, x.double(), cond, None, None, STEPS, shift=SHIFT, solver=solver))
    assert d1 < TOL, d1


# ---- 5. what a first-frame-replacement handle refuses -------------------------------------------------------------------------------
def test_refusals_on_the_handle(case):
    sd, x, t, cond = case
    L = _lib.lib()
    from fastgen_amd.networks.WanI2V.network import WanI2V

    net = WanI2V(**dict(dict(KW, **TI2V), r_timestep=True)).cuda().eval()
    gc, xg = _gpu_cond(cond), x.cuda()
    with torch.inference_mode():
        with pytest.raises(NotImplementedError, match="meanflow"):
            net.few_step_sample(xg, gc, [0.9, 0.5, 0.0], loop="meanflow")
        out = net(xg, t.cuda(), condition=gc, r=0.5 * t.cuda())  # (the r rows' frame 0 is zero as well: the call itself is served)
        assert torch.isfinite(out).all() and torch.equal(out[:, :, 0], gc["first_frame_cond"][:, :, 0])
    B, _, F, H, W = x.shape
    ws = net._ws(L.fg_wan_full_sampler_workspace_bytes(net._h, B, F, H, W), xg.device)
    sc = _lib.fg_wan_sampler_config()
    sc.t_scale, sc.net_pred_flow, sc.schedule = 1000.0, 1, _lib.FG_SCHEDULE_RF
    tl = (ctypes.c_double * 3)(0.9, 0.5, 0.0)
    res = torch.empty_like(xg)

    def run(loop):
        return L.fg_wan_full_sampler_run(net._h, ctypes.byref(sc), ptr(xg), tl, 2, _lib.SAMPLE_TYPES["ode"], _lib.LOOP_KINDS[loop], None,
                                         ctypes.c_uint64(0), ptr(res), B, F, H, W, ptr(ws), ws.numel(), 0, None)

    assert run("meanflow") == FG_EINVAL and b"first-frame-replacement" in L.fg_last_error()
    assert run("x0") == 0
    torch.cuda.synchronize()
    assert torch.equal(res[:, :, 0], gc["first_frame_cond"][:, :, 0])
    # another batch than the condition's
    assert L.fg_wan_full_sampler_run(net._h, ctypes.byref(sc), ptr(xg), tl, 2, _lib.SAMPLE_TYPES["ode"], _lib.LOOP_KINDS["x0"], None,
                                     ctypes.c_uint64(0), ptr(res), 1, F, H, W, ptr(ws), ws.numel(), 0, None) != 0
    # the chunked and causal entry points
    ts = torch.zeros(B * F, device="cuda")
    assert L.fg_wan_forward(net._h, ptr(xg), ptr(ts), ptr(res), B, F, H, W, 0, 0, ptr(ws), ws.numel(), None) == FG_EINVAL
    assert L.fg_wan_forward_block_causal(net._h, ptr(xg), ptr(ts), ptr(res), B, F, H, W, ptr(ws), ws.numel(), None) == FG_EINVAL
    gsc = _lib.fg_wan_sampler_config()
    gsc.t_scale, gsc.net_pred_flow, gsc.schedule = 1000.0, 1, _lib.FG_SCHEDULE_RF
    assert L.fg_wan_sampler_run(net._h, ctypes.byref(gsc), ptr(xg), tl, 2, _lib.SAMPLE_TYPES["ode"], None, None, ctypes.c_uint64(0), B, F, H, W,
                                ptr(ws), ws.numel(), 0, None) == FG_EINVAL


# ---- 6. FSDP2 -----------------------------------------------------------------------------------------------------------------------
def test_fsdp2_one_rank_mesh_equals_bare_module(case):
    import torch.distributed as dist
    from torch.distributed.device_mesh import init_device_mesh
    from torch.distributed.tensor import DTensor

    from fastgen_amd.methods.model import FastGenModel

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    created = False
    if not dist.is_initialized():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
        created = True
    try:
        mesh = init_device_mesh("cuda", (1,))
        sd, x, t, cond = case
        bare, net = _net(sd), _net(sd)
        net.fully_shard(mesh=mesh)
        assert all(isinstance(p, DTensor) for p in net.parameters())
        assert list(net.state_dict().keys()) == list(bare.state_dict().keys())
        gc, xg, tg = _gpu_cond(cond), x.cuda(), t.cuda()
        with torch.inference_mode():
            assert torch.equal(net(xg, tg, condition=gc), bare(xg, tg, condition=gc))
            kw = dict(student_sample_steps=2, t_list=[0.999, 0.5, 0.0], condition=gc, student_sample_type="ode")
            assert torch.equal(FastGenModel.generator_fn(net, xg, **kw), FastGenModel.generator_fn(bare, xg, **kw))
            neg = dict(gc, text_embeds=-gc["text_embeds"])
            assert torch.equal(net.sample(xg, gc, neg, num_steps=2), bare.sample(xg, gc, neg, num_steps=2))
    finally:
        if created:
            dist.destroy_process_group()
