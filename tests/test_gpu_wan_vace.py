"""`VACEWan` on the GPU (fg_wan_create_vace, fg_wan_set_vace_context, fg_wan_set_vace_scale and `Wan`'s entry points on that handle) on
the 3-block network `V.TINY` (2 heads, D 256, ffn 512, text_dim 128) with VACE layers (0, 2), video [2, 16, 5, 16, 24] (480 tokens per
sample: a ragged 128-query tile), 37 text tokens, a 96-channel context of 5 frames - or 3, so that two frames of the control stream are
padding -, context_scale [0.5, 1.5] and a skip_layers = [0] case.  PARITY UNPINNED (tests/wan_vace_ref.py).

TOL is the project's 2e-2 for this network family; tests/test_wan_vace_ref.py holds every mutant 5 x TOL from the fp64 oracle on the case
that exposes it.  The tap bounds are tests/test_gpu_wan_blocks.py's TOL (imported), per (sample, frame), on increments, with every
stage run by the fp64 oracle on the GPU's own stage input.

Measured on the MI355X (also in DESIGN.md section 10):
  forward against the fp64 oracle, relative L2: 5.3e-3 (5-frame context), 5.3e-3 (3-frame), 4.5e-3 (skip_layers = [0]); plain `Wan` of
    the same three blocks against its own fp64 oracle: 5.1e-3.  The mutants from the GPU output: hint_before_block 0.11,
    pad_after_proj_in 0.22, scale_ignored 0.39, main_block_modulation 0.41, no_proj_in_residual 0.53, no_hints 1.04,
    chain_from_hint 1.09, hint_by_layer_index 1.13.
  taps, worst (sample, frame), relative L2 / max: attn1 2.5e-3 / 4.6e-3, inc1 7.1e-3 / 1.0e-2, attn2 4.0e-3 / 6.4e-3, inc2 9.3e-3 /
    1.4e-2, ffn 7.7e-3 / 9.1e-3.
  fp8 against bf16: 2.5e-2; the bf16 network without its hints against the one with them: 1.02.
  guided sample (3 steps, g = 1.5) against the fp64 oracle: unipc 5.4e-3, euler 5.3e-3; with the two contexts swapped: 0.49."""
import ctypes
import socket

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks._engine import ptr
from fastgen_amd.networks.Wan import solvers
from oracle import wan_ref as R
import wan_full_ref as W
import wan_vace_ref as V
from test_gpu_wan_blocks import MUTANT_FACTOR, TOL as BLOCK_TOL

pytestmark = pytest.mark.gpu

KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=3)
TOL = 2e-2
FG_EINVAL, FG_ENOTREADY = 1, 2


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _net(sd, context_scale=V.SCALES, **kw):
    from fastgen_amd.networks.VaceWan.network import VACEWan

    net = VACEWan(**dict(KW, vace_layers=V.VACE_LAYERS, context_scale=context_scale, **kw))
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


def _plain(sd, **kw):
    from fastgen_amd.networks.Wan.network import Wan

    net = Wan(**dict(KW, time_cond_type="abs", **kw))
    net.load_state_dict({k: v for k, v in sd.items() if k in W.state_dict_shapes(V.TINY, kw.get("r_timestep", False))}, strict=True)
    return net.cuda().eval()


def _gpu_cond(cond):
    return {"text_embeds": cond["text"].cuda(), "vid_context": cond["ctx"].cuda()}


# ---- 1. forward against the oracle and away from its mutants ----------------------------------------------------------------------------
def test_forward_against_oracle_and_its_mutants():
    """Every case against the fp64 oracle; every mutant on the case that exposes it (tests/test_wan_vace_ref.py holds it 5 x TOL from
    the oracle there).  Also printed: plain `Wan` (the same three blocks) against its own oracle - the yardstick for VACE's distance."""
    net = None
    for name in V.CASES:
        sd, x, t, cond, skip = V.case(name)
        net = net or _net(sd)
        with torch.inference_mode():
            got = net(x.cuda(), t.cuda(), condition=_gpu_cond(cond), skip_layers=skip).cpu()
        d = _rel(got, V.WanVaceRef(sd, V.TINY, torch.float64, context_scale=V.SCALES).forward(x, t, cond, skip_layers=skip))
        print("vace forward vs fp64 oracle", name, d)
        assert torch.isfinite(got).all() and d < TOL, (name, d)
        for m in (m for m in V.MUTANTS if V.EXPOSED_BY[m] == name):
            dm = _rel(got, V.WanVaceRef(sd, V.TINY, torch.float64, context_scale=V.SCALES, mutant=m).forward(x, t, cond, skip_layers=skip))
            print("  mutant", m, dm)
            assert dm > 5 * TOL, (m, dm)
    sd, x, t, cond, _ = V.case("full")
    plain_net = _plain(sd)
    with torch.inference_mode():
        x0 = net(x.cuda(), t.cuda(), condition=_gpu_cond(cond), fwd_pred_type="x0").cpu()
        flow = net(x.cuda(), t.cuda(), condition=_gpu_cond(cond)).cpu()
        plain = plain_net(x.cuda(), t.cuda(), condition=cond["text"].cuda()).cpu()
    assert _rel(x0, x - t.view(-1, 1, 1, 1, 1).float() * flow) < 1e-6  # (the schedule's flow -> x0 conversion)
    plain_sd = {k: v for k, v in sd.items() if k in W.state_dict_shapes(V.TINY)}
    dp = _rel(plain, W.WanFullRef(plain_sd, V.TINY, torch.float64).forward(x, t, cond["text"]))
    print("plain Wan (3 layers, same weights) vs its fp64 oracle", dp)
    assert dp < TOL, dp


# ---- 2. the taps of the control stream and the first place a hint is visible -------------------------------------------------------------
def _granules(got, want, B, F):
    """worst (relative L2, max |err| / max |ref|) over the (sample, frame) granules of two [B, L, D] tensors"""
    g, w = got.double().view(B, F, -1), want.double().view(B, F, -1)
    return float(((g - w).norm(dim=2) / w.norm(dim=2)).max()), float(((g - w).abs().amax(dim=2) / w.abs().amax(dim=2)).max())


def test_taps_of_the_vace_blocks_and_the_first_injection_against_fp64():
    sd, x, t, cond, _ = V.case("full")
    net = _net(sd)
    B, _, F, H, Wd = x.shape
    dev, L = torch.device("cuda"), _lib.lib()
    xg, gc = x.cuda(), _gpu_cond(cond)
    M, D = F * (H // 2) * (Wd // 2), 256
    with torch.inference_mode():
        net._prepare(xg, "x_t", gc["vid_context"])
        ws = net._ws(L.fg_wan_full_workspace_bytes(net._h, B, F, H, Wd), dev)
        net._set_text(gc["text_embeds"], B, dev, ws)
    ts = (1000.0 * t.float()).view(B, 1).expand(B, F).contiguous().cuda()
    out = torch.empty_like(xg)
    names = ("attn1", "x_attn1", "attn2", "x_attn2", "x_ffn")
    blocks = (0, 1, 3, 4)  # main block 0 (its x_ffn: what hint 0 joins), main block 1 (x_attn1), VACE blocks 0 and 1
    bufs = {i: {k: torch.full((B, M, D), float("nan"), device=dev) for k in names} for i in blocks}
    taps = (_lib.fg_wan_block_taps * len(blocks))()
    for tp, i in zip(taps, blocks):
        for k in names:
            setattr(tp, k, bufs[i][k].data_ptr())
    tokens, tproj, ctx_in = torch.empty(B, M, D, device=dev), torch.empty(B * F, 6 * D, device=dev), torch.empty(B, M, D, device=dev)
    _lib.check(L.fg_wan_forward_full_features(net._h, ptr(xg), ptr(ts), None, ptr(out), B, F, H, Wd, None, 0, (ctypes.c_int * 4)(*blocks), taps, 4,
                                              ptr(tokens), None, ptr(tproj), ptr(ws), ws.numel(), None))
    _lib.check(L.fg_wan_vace_context_read(net._h, ptr(ctx_in), None))
    torch.cuda.synchronize()
    plain_out = torch.empty_like(xg)
    _lib.check(L.fg_wan_forward_full(net._h, ptr(xg), ptr(ts), None, ptr(plain_out), B, F, H, Wd, None, 0, ptr(ws), ws.numel(), None))
    torch.cuda.synchronize()
    assert torch.equal(out, plain_out)  # the tapped call computes what the untapped one does
    ref = V.WanVaceRef(sd, V.TINY, torch.float64)
    ref.p = {k: v.cuda() for k, v in ref.p.items()}
    p, cfg = ref.p, V.TINY
    cos, sin = R.rope_for_chunk(cfg, F, H // 2, Wd // 2, 0, torch.float64)
    cos, sin = cos.cuda(), sin.cuda()
    text = R.text_embedding(p, gc["text_embeds"].double())
    tp64 = tproj.double()
    worst, bad = {}, []

    def check(key, got, want, where):
        e = _granules(got, want, B, F)
        worst[key] = tuple(max(a, b) for a, b in zip(worst.get(key, (0.0, 0.0)), e))
        if e[0] > BLOCK_TOL[key][0] or e[1] > BLOCK_TOL[key][1]:
            bad.append((where, key, e))
        return e

    def stages(i, x_in, b, where, mod_from=None, mutant=False):
        """block i, every stage run in fp64 on the GPU's own stage input.  mutant: the oracle is a wrong one (another block's
        modulation table, another input) - only inc1's distance is returned, relative L2 in multiples of its bound."""
        mod = R.modulation(p, i if mod_from is None else mod_from, tp64, B, F)
        q, k, v = R.self_attn_qkv(p, cfg, i, x_in, mod, cos, sin)
        att1 = R.sdpa(q, k, v).flatten(2)
        inc1 = R.self_attn_out(p, i, x_in, att1, mod) - x_in
        if mutant:
            return _granules(b["x_attn1"].double() - x_in, inc1, B, F)[0] / BLOCK_TOL["inc1"][0]
        check("attn1", b["attn1"], att1, where)
        check("inc1", b["x_attn1"].double() - x_in, inc1, where)
        xa1 = b["x_attn1"].double()
        att2, xa2 = R.cross_attn(p, cfg, i, xa1, *R.cross_kv(p, cfg, i, text))
        check("attn2", b["attn2"], att2.flatten(2), where)
        check("inc2", b["x_attn2"].double() - xa1, xa2 - xa1, where)
        xa2g = b["x_attn2"].double()
        check("ffn", b["x_ffn"].double() - xa2g, R.ffn(p, cfg, i, xa2g, mod) - xa2g, where)

    # VACE block 0 starts from c = ctx_in + x0, rounded once; VACE block 1 from block 0's stream (not from its hint)
    c0 = (ctx_in + tokens).bfloat16().double()
    stages(V._VB + 0, c0, bufs[3], "vace block 0")
    stages(V._VB + 1, bufs[3]["x_ffn"].double(), bufs[4], "vace block 1")
    assert stages(V._VB + 0, c0, bufs[3], "", mod_from=0, mutant=True) >= MUTANT_FACTOR  # the MAIN block's scale_shift_table
    assert stages(V._VB + 0, ctx_in.double(), bufs[3], "", mutant=True) >= MUTANT_FACTOR  # no x0 behind proj_in
    hint0 = R._lin(p, bufs[3]["x_ffn"].double(), "vace_blocks.0.proj_out")
    assert stages(V._VB + 1, hint0, bufs[4], "", mutant=True) >= MUTANT_FACTOR  # the chain continued from the hint
    # main block 1's x_attn1 is the first place hint 0 (scale 0.5) is visible: its increment over main block 0's x_ffn holds the hint
    xf0 = bufs[0]["x_ffn"].double()

    def first_visible(scale):
        x_in = xf0 + scale * hint0
        mod = R.modulation(p, 1, tp64, B, F)
        q, k, v = R.self_attn_qkv(p, cfg, 1, x_in, mod, cos, sin)
        return R.self_attn_out(p, 1, x_in, R.sdpa(q, k, v).flatten(2), mod) - xf0

    got_inc = bufs[1]["x_attn1"].double() - xf0
    check("inc1", got_inc, first_visible(V.SCALES[0]), "main block 1 behind hint 0")
    for name, s in (("no_hints", 0.0), ("scale_ignored", 1.0)):
        assert _granules(got_inc, first_visible(s), B, F)[0] >= MUTANT_FACTOR * BLOCK_TOL["inc1"][0], name
    print("vace taps vs fp64 (relative L2 / max)", {k: tuple(round(v, 5) for v in e) for k, e in worst.items()})
    assert not bad, bad
    # a VACE block that the call's skip_layers keep from running cannot be tapped; on a plain handle the index does not exist
    one = (_lib.fg_wan_block_taps * 1)()
    rc = L.fg_wan_forward_full_features(net._h, ptr(xg), ptr(ts), None, ptr(out), B, F, H, Wd, (ctypes.c_int * 1)(0), 1, (ctypes.c_int * 1)(4), one, 1,
                                        None, None, None, ptr(ws), ws.numel(), None)
    assert rc == FG_EINVAL and b"does not run" in L.fg_last_error()


# ---- 3. bit-equalities with the plain network ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_zero_scale_and_zero_proj_out_are_plain_wan(mode):
    sd, x, t, cond, _ = V.case("short")
    xg, tg, gc = x.cuda(), t.cuda(), _gpu_cond(cond)
    zero = {k: (torch.zeros_like(v) if ".proj_out." in k and "vace_blocks" in k else v) for k, v in sd.items()}
    plain, net = _plain(sd, compute_dtype=mode), _net(sd, compute_dtype=mode)
    unscaled, silent = _net(sd, context_scale=0.0, compute_dtype=mode), _net(zero, compute_dtype=mode)
    with torch.inference_mode():
        want = plain(xg, tg, condition=gc["text_embeds"])
        hinted = net(xg, tg, condition=gc)
        assert torch.isfinite(want).all() and not torch.equal(hinted, want)
        assert torch.equal(unscaled(xg, tg, condition=gc), want)
        assert torch.equal(silent(xg, tg, condition=gc), want)
        # the scales are read at every call: the same module, new scales, no new handle
        net.context_scale = [0.0, 0.0]
        assert torch.equal(net(xg, tg, condition=gc), want)
        net.context_scale = V.SCALES
        assert torch.equal(net(xg, tg, condition=gc), hinted)


# ---- 4. fp8 ---------------------------------------------------------------------------------------------------------------------------------
def test_fp8_with_a_control_video():
    sd, x, t, cond, _ = V.case("full")
    xg, tg, gc = x.cuda(), t.cuda(), _gpu_cond(cond)
    bf16, fp8, bare = _net(sd), _net(sd, compute_dtype="fp8"), _net(sd, context_scale=0.0)
    with torch.inference_mode():
        a, b = bf16(xg, tg, condition=gc), fp8(xg, tg, condition=gc)
        c = bare(xg, tg, condition=gc)  # the bf16 network without its hints
    print("vace fp8 vs bf16", _rel(b, a), "no hints vs bf16", _rel(c, a))
    assert torch.isfinite(b).all() and not torch.equal(a, b) and _rel(b, a) < _rel(c, a)


# ---- 5. the fused loops ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", ["x0", "meanflow"])
def test_fused_loops_equal_the_generic_loops_and_replay_on_new_contents(loop, monkeypatch):
    from fastgen_amd.methods.consistency_model.mean_flow import MeanFlowModel
    from fastgen_amd.methods.model import FastGenModel

    cls = FastGenModel if loop == "x0" else MeanFlowModel
    sd, x, _, cond, _ = V.case("short", seed=85, r_timestep=loop == "meanflow")
    net = _net(sd, r_timestep=loop == "meanflow")
    gc = _gpu_cond(cond)
    g = torch.Generator().manual_seed(86)
    noise, eps = x.cuda(), torch.randn((2, *V.SHAPE), generator=g).cuda()
    sch = net.noise_scheduler

    def per_step(c, kind):
        tl = sch.get_t_list(3, device="cuda")
        pending = [e for e in eps]
        monkeypatch.setattr(torch, "randn_like", lambda x_, **kw: pending.pop(0))
        with torch.inference_mode():
            out = cls._student_sample_loop(net, sch.latents(noise, tl[0]), tl, condition=c, student_sample_type=kind)
        monkeypatch.undo()
        return out

    kw = dict(student_sample_steps=3, eps=eps)
    for kind in ("sde", "ode"):
        want = per_step(gc, kind)
        got = cls.generator_fn(net, noise, student_sample_type=kind, condition=gc, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, want), kind
        assert torch.equal(cls.generator_fn(net, noise, student_sample_type=kind, condition=gc, use_graph=False, **kw), want), kind
    # a new context at the same shape, then new scales: the cached graph, the new result
    gc2 = dict(gc, vid_context=torch.randn(cond["ctx"].shape, generator=g).cuda())
    captures, launches = _lib.graph_stats()
    got2 = cls.generator_fn(net, noise, student_sample_type="ode", condition=gc2, **kw)
    assert _lib.graph_stats() == (captures, launches + 1), "a new context at the same shape captured a new graph"
    assert torch.equal(got2, per_step(gc2, "ode")) and not torch.equal(got2, want)
    net.context_scale = [1.0, 0.25]
    got3 = cls.generator_fn(net, noise, student_sample_type="ode", condition=gc2, **kw)
    assert _lib.graph_stats() == (captures, launches + 2), "new scales captured a new graph"
    assert torch.equal(got3, per_step(gc2, "ode")) and not torch.equal(got3, got2)


# ---- 6. sample() ----------------------------------------------------------------------------------------------------------------------------
def _per_call_guided_loop(net, noise, cond, neg, guidance_scale, num_steps, shift, solver):
    """`VACEWan.sample` as separate calls: per step one forward of the stacked batch [x; x] against the stacked dicts, then the torch
    mirror of the update kernel (tests/test_gpu_wan_full.py's)."""
    B, sch = noise.shape[0], net.noise_scheduler
    both = {k: torch.cat([cond[k], neg[k]]) for k in cond}
    sig = solvers.flow_shift_sigmas(num_steps, shift)
    tab = solvers.multistep_table(sig, solver, guidance_scale)
    t_net = sch.safe_clamp(torch.floor(sig[:-1] * 1000.0) / 1000.0, min=sch.min_t, max=sch.max_t).cuda()
    cur, x_last, m_prev = sch.latents(noise, t_net[0]), None, None
    for i in range(num_steps):
        v = net(torch.cat([cur, cur]), t_net[i].expand(2 * B), condition=both, fwd_pred_type="flow")
        cur, x_last, m_prev = solvers.multistep_update(tab[i], cur, v[:B], x_last, m_prev, v_uncond=v[B:])
    return cur


@pytest.mark.parametrize("solver", ["unipc", "euler"])
def test_guided_sample(solver):
    G, STEPS, SHIFT = 1.5, 3, 16.0  # (g = 1.5: tests/test_gpu_wan_full.py's oracle case; shift 16: this class's default)
    sd, x, _, cond, _ = V.case("short", seed=87)
    g = torch.Generator().manual_seed(88)
    neg = {"text": -cond["text"], "ctx": torch.cat([torch.randn(2, 32, 3, 16, 24, generator=g), torch.ones(2, 64, 3, 16, 24)], dim=1)}
    net = _net(sd)
    gc, gn, noise = _gpu_cond(cond), _gpu_cond(neg), x.cuda()
    kw = dict(guidance_scale=G, num_steps=STEPS, solver=solver)
    with torch.inference_mode():
        want = _per_call_guided_loop(net, noise, gc, gn, G, STEPS, SHIFT, solver)
        got = net.sample(noise, gc, gn, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, want)
        assert torch.equal(net.sample(noise, gc, gn, use_graph=False, **kw), want)
        swapped = net.sample(noise, dict(gc, vid_context=gn["vid_context"]), dict(gn, vid_context=gc["vid_context"]), **kw)
        assert not torch.equal(swapped, got)
    ref = V.WanVaceRef(sd, V.TINY, dtype=torch.float64, context_scale=V.SCALES)
    oracle = V.guided_sample(ref, x.double(), cond, neg, G, STEPS, shift=SHIFT, solver=solver)
    d, dsw = _rel(got.cpu(), oracle), _rel(swapped.cpu(), oracle)
    print("vace guided sample vs fp64 oracle", solver, d, "contexts swapped", dsw)
    assert d < TOL and dsw > 5 * TOL, (d, dsw)


# ---- 7. FSDP2 ---------------------------------------------------------------------------------------------------------------------------------
def test_fsdp2_one_rank_mesh_equals_bare_module():
    """`fully_shard` on a 1-rank mesh, as tests/test_gpu_wan_full.py's case for `Wan`: the VACE blocks and vace_patch_embedding ride in
    the root group (the reference's fully_shard wraps `transformer.blocks` only)."""
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
        sd, x, t, cond, _ = V.case("short", seed=89)
        bare, net = _net(sd), _net(sd)
        net.fully_shard(mesh=mesh)
        assert all(isinstance(p, DTensor) for p in net.parameters())
        assert list(net.state_dict().keys()) == list(bare.state_dict().keys()) == list(V.state_dict_shapes(V.TINY))
        gc, xg, tg = _gpu_cond(cond), x.cuda(), t.cuda()
        with torch.inference_mode():
            assert torch.equal(net(xg, tg, condition=gc), bare(xg, tg, condition=gc))
            assert all(isinstance(p, DTensor) for p in net.parameters())
            kw = dict(student_sample_steps=2, t_list=[0.999, 0.5, 0.0], condition=gc, student_sample_type="ode")
            assert torch.equal(FastGenModel.generator_fn(net, xg, **kw), FastGenModel.generator_fn(bare, xg, **kw))
            neg = dict(gc, text_embeds=-gc["text_embeds"])
            assert torch.equal(net.sample(xg, gc, neg, num_steps=2), bare.sample(xg, gc, neg, num_steps=2))
    finally:
        if created:
            dist.destroy_process_group()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_gpu():
    sd, x, t, cond, _ = V.case("full")
    net = _net(sd)
    xg, tg, gc = x.cuda(), t.cuda(), _gpu_cond(cond)
    B, _, F, H, Wd = x.shape
    dev, L = torch.device("cuda"), _lib.lib()
    with torch.inference_mode():
        net._bind(dev)
        ws = net._ws(L.fg_wan_full_workspace_bytes(net._h, B, F, H, Wd), dev)
        net._set_text(gc["text_embeds"], B, dev, ws)
        ts = (1000.0 * t.float()).view(B, 1).expand(B, F).contiguous().cuda()
        out = torch.empty_like(xg)
        args = (net._h, ptr(xg), ptr(ts), None, ptr(out), B, F, H, Wd, None, 0, ptr(ws), ws.numel(), None)
        assert L.fg_wan_forward_full(*args) == FG_ENOTREADY and b"no VACE context" in L.fg_last_error()  # packed, text set, no context
        # a context for another batch does not serve this call
        c1 = gc["vid_context"][:1].contiguous()
        wsv = torch.empty(L.fg_wan_vace_context_workspace_bytes(net._h, 1, F, H, Wd), dtype=torch.uint8, device=dev)
        _lib.check(L.fg_wan_set_vace_context(net._h, ptr(c1), 1, F, F, H, Wd, ptr(wsv), wsv.numel(), None))
        assert L.fg_wan_forward_full(*args) == FG_ENOTREADY
        assert L.fg_wan_forward(net._h, ptr(xg), ptr(ts), ptr(out), B, 1, H, Wd, 0, 0, ptr(ws), ws.numel(), None) == FG_EINVAL
        assert b"not implemented for a VACE handle" in L.fg_last_error()
        for bad, word in ((torch.zeros(B, 96, F, H, Wd + 2), "height and width"), (torch.zeros(B, 96, F + 1, H, Wd), "more frames")):
            with pytest.raises(ValueError, match=word):
                net(xg, tg, condition=dict(gc, vid_context=bad.cuda()))
        net.context_scale = [1.0]
        with pytest.raises(ValueError, match=r"Length of `control_hidden_states_scale` 1 does not match number of layers 2\."):
            net(xg, tg, condition=gc)
        net.context_scale = V.SCALES
        assert torch.isfinite(net(xg, tg, condition=gc)).all()  # ... and the module recovers
        # a pack group that holds some of a VACE block's parameters is refused (the block is packed whole, with the root group); one
        # that holds none of them leaves the VACE blocks alone
        assert L.fg_wan_pack_group(net._h, b"transformer.vace_blocks.0.attn1.", None, None) == FG_ENOTREADY and b"packed whole" in L.fg_last_error()
        assert L.fg_wan_pack_group(net._h, b"transformer.vace_blocks.1.", b"transformer.vace_blocks.1.proj_out.", None) == FG_ENOTREADY
        want = net(xg, tg, condition=gc)
        _lib.check(L.fg_wan_pack_group(net._h, b"transformer.blocks.1.", None, None))
        net._forget_text()  # (packing invalidates the text and the context on the handle)
        assert torch.equal(net(xg, tg, condition=gc), want)
