"""`WanI2V` on the GPU (fg_wan_create_i2v, fg_wan_set_i2v_cond and `Wan`'s entry points on that handle) on the 2-block network
`I.TINY` (2 heads, D 256, ffn 512, text_dim 128, image_dim 128), video [2, 16, 5, 16, 24] (480 tokens per sample: a ragged 128-query
tile), 37 text tokens and 257 image tokens (ragged key tiles in both contexts).  PARITY UNPINNED (tests/wan_i2v_ref.py).

Measured on the MI355X:
  forward against the fp32 oracle, relative L2: 4.5e-3 (TOL 2e-2, tests/test_gpu_wan_full.py's for this network and arithmetic);
    the mutants from the GPU output: joint_softmax 0.39, no_image 0.64, no_norm_added_k 0.34, mask_every_frame 0.25,
    cond_before_mask 0.37, neighbour_first_frame 0.34.
  taps against the fp64 oracle on the GPU's own block input (x_attn1), relative L2, worst over the two blocks: attn2 4.1e-3,
    x_attn2 - x_attn1 5.6e-3: TAP_BOUND = twice these.
  fp8 against bf16: 2.8e-2; the bf16 call without the image tokens against the one with them: 0.61.
  guided sample (3 steps, g = 1.5) against the fp64 oracle: unipc 3.8e-3, euler 3.7e-3; with the two first frames swapped: 0.82."""
import ctypes
import socket

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks._engine import ptr
from fastgen_amd.networks.Wan import solvers
from oracle import wan_ref as R
import wan_i2v_ref as I

pytestmark = pytest.mark.gpu

KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2)
TOL = 2e-2
TAP_BOUND = {"attn2": 2 * 4.1e-3, "inc": 2 * 5.6e-3}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _net(sd, image_dim=I.TINY_IMAGE_DIM, **kw):
    from fastgen_amd.networks.WanI2V.network import WanI2V

    net = WanI2V(**dict(KW, image_dim=image_dim, **kw))
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


def _gpu_cond(cond):
    out = {"text_embeds": cond["text"].cuda(), "first_frame_cond": cond["ff"].cuda()}
    if "image" in cond:
        out["encoder_hidden_states_image"] = cond["image"].cuda()
    return out


# ---- 1. forward against the oracle and away from its mutants ----------------------------------------------------------------------------
def test_forward_against_oracle_and_its_mutants():
    """tests/test_wan_i2v_ref.py holds every mutant at least 5 x TOL from the oracle for these inputs."""
    sd, x, t, cond = I.case()
    net = _net(sd)
    with torch.inference_mode():
        got = net(x.cuda(), t.cuda(), condition=_gpu_cond(cond)).cpu()
        x0 = net(x.cuda(), t.cuda(), condition=_gpu_cond(cond), fwd_pred_type="x0").cpu()
    d = _rel(got, I.WanI2VRef(sd, I.TINY).forward(x, t, cond))
    print("i2v forward vs oracle", d)
    assert torch.isfinite(got).all() and d < TOL, d
    assert _rel(x0, x - t.view(-1, 1, 1, 1, 1).float() * got) < 1e-6  # (the schedule's flow -> x0 conversion on the 16 latent channels)
    for m in I.MUTANTS:
        dm = _rel(got, I.WanI2VRef(sd, I.TINY, mutant=m).forward(x, t, cond))
        print("  mutant", m, dm)
        assert dm > 5 * TOL, (m, dm)


# ---- 2. the cross-attention taps ------------------------------------------------------------------------------------------------------
def test_cross_attention_taps_against_fp64_on_the_gpus_own_block_input():
    sd, x, t, cond = I.case()
    net = _net(sd)
    B, _, F, H, W = x.shape
    dev, L = torch.device("cuda"), _lib.lib()
    xg, gc = x.cuda(), _gpu_cond(cond)
    M, D = F * (H // 2) * (W // 2), 256
    with torch.inference_mode():
        net._prepare(xg, "x_t", gc["first_frame_cond"], gc["encoder_hidden_states_image"])
        ws = net._ws(L.fg_wan_full_workspace_bytes(net._h, B, F, H, W), dev)
        net._set_text(gc["text_embeds"], B, dev, ws)
    ts = (1000.0 * t.float()).view(B, 1).expand(B, F).contiguous().cuda()
    out = torch.empty_like(xg)
    bufs = [{k: torch.empty(B, M, D, device=dev) for k in ("x_attn1", "attn2", "x_attn2")} for _ in range(2)]
    taps = (_lib.fg_wan_block_taps * 2)()
    for tp, b in zip(taps, bufs):
        tp.x_attn1, tp.attn2, tp.x_attn2 = b["x_attn1"].data_ptr(), b["attn2"].data_ptr(), b["x_attn2"].data_ptr()
    _lib.check(L.fg_wan_forward_full_features(net._h, ptr(xg), ptr(ts), None, ptr(out), B, F, H, W, None, 0, (ctypes.c_int * 2)(0, 1), taps, 2, None,
                                              None, None, ptr(ws), ws.numel(), None))
    torch.cuda.synchronize()
    p = {k[len("transformer."):]: v.double().cuda() for k, v in sd.items()}
    ctx = R.text_embedding(p, gc["text_embeds"].double())
    tok = I.image_embedding(p, gc["encoder_hidden_states_image"].double())
    worst = {"attn2": 0.0, "inc": 0.0}
    for i, b in enumerate(bufs):
        hs = b["x_attn1"].double()
        k2, v2 = R.cross_kv(p, I.TINY, i, ctx)
        ki, vi = I.img_kv(p, I.TINY, i, tok)
        att, new = I.cross_attn_i2v(p, I.TINY, i, hs, k2, v2, ki, vi)
        got_inc = b["x_attn2"].double() - hs
        e = {"attn2": _rel(b["attn2"], att), "inc": _rel(got_inc, new - hs)}
        for k_ in worst:
            worst[k_] = max(worst[k_], e[k_])
        for name, kw in (("joint_softmax", dict(ki=ki, vi=vi, joint=True)), ("no_image", dict())):
            ma, mn = I.cross_attn_i2v(p, I.TINY, i, hs, k2, v2, **kw)
            assert _rel(b["attn2"], ma) >= 5 * TAP_BOUND["attn2"] and _rel(got_inc, mn - hs) >= 5 * TAP_BOUND["inc"], (name, i)
    print("i2v taps vs fp64", worst)
    assert worst["attn2"] <= TAP_BOUND["attn2"] and worst["inc"] <= TAP_BOUND["inc"], worst


# ---- 3. no image context: the plain network on the concatenated input ------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp8"])
@pytest.mark.parametrize("how", ["image_dim_0", "key_absent"])
def test_without_an_image_context_it_is_wan_on_the_concatenated_input(how, mode):
    from fastgen_amd.networks.Wan.network import Wan

    image_dim = 0 if how == "image_dim_0" else I.TINY_IMAGE_DIM
    sd, x, t, cond = I.case(image_dim=image_dim)
    cond.pop("image", None)
    net = _net(sd, image_dim=image_dim, compute_dtype=mode)
    plain = Wan(**dict(KW, in_channels=36, compute_dtype=mode))
    plain.load_state_dict({k: v for k, v in sd.items() if k in dict(R.state_dict_shapes(I.TINY))}, strict=True)
    plain = plain.cuda().eval()
    cat = torch.cat([x, I.mask_first_frame(x.shape[0], *x.shape[2:]), cond["ff"]], dim=1)
    with torch.inference_mode():
        got = net(x.cuda(), t.cuda(), condition=_gpu_cond(cond))
    # (`Wan.forward` shapes its output like its 36-channel input; the plain network's 16-channel flow is taken from the library call)
    want = _raw_forward(plain, cat.cuda(), t, cond["text"].cuda())
    assert torch.isfinite(got).all() and torch.equal(got, want)


def _raw_forward(net, x, t, text):
    B, _, F, H, W = x.shape
    dev, L = x.device, _lib.lib()
    with torch.inference_mode():
        net._bind(dev)
        ws = net._ws(L.fg_wan_full_workspace_bytes(net._h, B, F, H, W), dev)
        net._set_text(text, B, dev, ws)
    ts = (1000.0 * t.float()).view(B, 1).expand(B, F).contiguous().cuda()
    out = torch.empty(B, 16, F, H, W, device=dev)
    _lib.check(L.fg_wan_forward_full(net._h, ptr(x.contiguous()), ptr(ts), None, ptr(out), B, F, H, W, None, 0, ptr(ws), ws.numel(), None))
    torch.cuda.synchronize()
    return out


# ---- 4. fp8 with an image context ---------------------------------------------------------------------------------------------------------
def test_fp8_with_an_image_context():
    sd, x, t, cond = I.case()
    gc = _gpu_cond(cond)
    no_img = {k: v for k, v in gc.items() if k != "encoder_hidden_states_image"}
    bf16, fp8 = _net(sd), _net(sd, compute_dtype="fp8")
    with torch.inference_mode():
        a, b, c = bf16(x.cuda(), t.cuda(), condition=gc), fp8(x.cuda(), t.cuda(), condition=gc), bf16(x.cuda(), t.cuda(), condition=no_img)
    print("i2v fp8 vs bf16", _rel(b, a), "no image vs bf16", _rel(c, a))
    assert torch.isfinite(b).all() and not torch.equal(a, b) and _rel(b, a) < _rel(c, a)


# ---- 5. the fused x0 loop -----------------------------------------------------------------------------------------------------------------
def test_fused_x0_loop_equals_the_generic_loop_and_replays_on_new_contents(monkeypatch):
    from fastgen_amd.methods.model import FastGenModel

    sd, x, _, cond = I.case(seed=73)
    net = _net(sd)
    gc = _gpu_cond(cond)
    g = torch.Generator().manual_seed(74)
    noise, eps = x.cuda(), torch.randn((2, *I.SHAPE), generator=g).cuda()
    sch = net.noise_scheduler

    def per_step(c, kind):
        tl = sch.get_t_list(3, device="cuda")
        pending = [e for e in eps]
        monkeypatch.setattr(torch, "randn_like", lambda x_, **kw: pending.pop(0))
        with torch.inference_mode():
            out = FastGenModel._student_sample_loop(net, sch.latents(noise, tl[0]), tl, condition=c, student_sample_type=kind)
        monkeypatch.undo()
        return out

    kw = dict(student_sample_steps=3, eps=eps)
    for kind in ("sde", "ode"):
        want = per_step(gc, kind)
        got = FastGenModel.generator_fn(net, noise, student_sample_type=kind, condition=gc, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, want), kind
        assert torch.equal(FastGenModel.generator_fn(net, noise, student_sample_type=kind, condition=gc, use_graph=False, **kw), want), kind
    # new first-frame contents and new image tokens at the same shapes: the cached graph, the new result
    gc2 = dict(gc, first_frame_cond=torch.randn(I.SHAPE, generator=g).cuda(),
               encoder_hidden_states_image=torch.randn(2, I.IMAGE_LEN, I.TINY_IMAGE_DIM, generator=g).cuda())
    captures, launches = _lib.graph_stats()
    got2 = FastGenModel.generator_fn(net, noise, student_sample_type="ode", condition=gc2, **kw)
    assert _lib.graph_stats() == (captures, launches + 1), "new contents at the same shapes captured a new graph"
    want2 = per_step(gc2, "ode")
    assert torch.equal(got2, want2) and not torch.equal(got2, want)


# ---- 6. sample() ----------------------------------------------------------------------------------------------------------------------------
def _per_call_guided_loop(net, noise, cond, neg, guidance_scale, num_steps, shift, solver):
    """`WanI2V.sample` as separate calls: per step one forward of the stacked batch [x; x] against the stacked dicts, then the torch
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
    G, STEPS, SHIFT = 1.5, 3, 3.0  # (g = 1.5: tests/test_gpu_wan_full.py's oracle case; the flows' errors scale with g and g - 1)
    sd, x, _, cond = I.case(seed=75)
    g = torch.Generator().manual_seed(76)
    neg = {"text": -cond["text"], "ff": torch.randn(I.SHAPE, generator=g), "image": torch.randn(2, I.IMAGE_LEN, I.TINY_IMAGE_DIM, generator=g)}
    net = _net(sd)
    gc, gn, noise = _gpu_cond(cond), _gpu_cond(neg), x.cuda()
    kw = dict(guidance_scale=G, num_steps=STEPS, solver=solver)
    with torch.inference_mode():
        want = _per_call_guided_loop(net, noise, gc, gn, G, STEPS, SHIFT, solver)
        got = net.sample(noise, gc, gn, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, want)
        assert torch.equal(net.sample(noise, gc, gn, use_graph=False, **kw), want)
        swapped = net.sample(noise, dict(gc, first_frame_cond=gn["first_frame_cond"]), dict(gn, first_frame_cond=gc["first_frame_cond"]), **kw)
        assert not torch.equal(swapped, got)
    ref = I.WanI2VRef(sd, I.TINY, dtype=torch.float64)
    oracle = I.guided_sample(ref, x.double(), cond, neg, G, STEPS, shift=SHIFT, solver=solver)
    d, dsw = _rel(got.cpu(), oracle), _rel(swapped.cpu(), oracle)
    print("i2v guided sample vs oracle", solver, d, "first frames swapped", dsw)
    assert d < TOL and dsw > 5 * TOL, (d, dsw)


# ---- 7. FSDP2 ---------------------------------------------------------------------------------------------------------------------------------
def test_fsdp2_one_rank_mesh_equals_bare_module():
    """`fully_shard` on a 1-rank mesh, as tests/test_gpu_wan_full.py's case for `Wan`: the image embedder rides in the root group, the
    image projections in their blocks' groups."""
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
        sd, x, t, cond = I.case(seed=77)
        bare, net = _net(sd), _net(sd)
        net.fully_shard(mesh=mesh)
        assert all(isinstance(p, DTensor) for p in net.parameters())
        assert list(net.state_dict().keys()) == list(bare.state_dict().keys())
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
