"""The bidirectional video DiT `Wan` on the GPU (fg_wan_forward_full, fg_wan_full_sampler_run, fg_wan_full_guided_sampler_run) on the
2-block network `R.TINY` and two video shapes: [2,16,5,16,24] (480 tokens per sample: a ragged 128-query tile, batch 2) and
[1,16,12,16,24] (1152 tokens: more than 1024 keys, and more frames than TINY's total_num_frames = 6).  Bit-equal to the block-causal
call with one chunk; against the fp32 oracle tests/wan_full_ref.py and away from its mutants; the fused loops bit-equal to the generic
loops over `Wan.forward`; `sample()`; the causal module beside it; FSDP2 on a one-rank mesh.  PARITY UNPINNED."""
import functools
import socket

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks.Wan import solvers
from oracle import wan_ref as R
import wan_full_ref as W

pytestmark = pytest.mark.gpu

KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2)
TOL = 2e-2  # tests/test_wan.py::test_block_causal_call_against_oracle's, for this network and arithmetic


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _wan(sd, **kw):
    from fastgen_amd.networks.Wan.network import Wan

    net = Wan(**dict(KW, **kw))
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


def _causal(sd, frames, chunk=None, **kw):
    from fastgen_amd.networks.Wan.network_causal import CausalWan

    net = CausalWan(chunk_size=chunk or frames, total_num_frames=frames, **dict(KW, **kw))
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


def _inputs(shape_key, seed):
    shp = W.SHAPES[shape_key]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shp, generator=g)
    text = torch.randn(shp[0], 24, 128, generator=g)
    t = torch.tensor([0.8, 0.45][: shp[0]], dtype=torch.float64)
    return x, t, text


# ---- 1. the same launches as the block-causal call with one chunk ----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp8"])
@pytest.mark.parametrize("shape_key", ["ragged", "long"])
def test_forward_is_the_block_causal_call_with_one_chunk(shape_key, mode):
    sd = R.random_state_dict(R.TINY, 31)
    x, t, text = _inputs(shape_key, 32)
    net, causal = _wan(sd, compute_dtype=mode), _causal(sd, x.shape[2], compute_dtype=mode)
    with torch.inference_mode():
        got = net(x.cuda(), t.cuda(), condition=text.cuda())
        want = causal(x.cuda(), t.cuda(), condition=text.cuda(), is_ar=False)
        assert torch.isfinite(got).all() and torch.equal(got, want)
        x0 = net(x.cuda(), t.cuda(), condition=text.cuda(), fwd_pred_type="x0")
        assert torch.equal(x0, causal(x.cuda(), t.cuda(), condition=text.cuda(), is_ar=False, fwd_pred_type="x0"))
        assert not torch.equal(x0, got)


# ---- 2. against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape_key", ["ragged", "long"])
def test_forward_against_oracle(shape_key):
    sd = R.random_state_dict(R.TINY, 33)
    x, t, text = _inputs(shape_key, 34)
    net, ref = _wan(sd), W.WanFullRef(sd, R.TINY)
    with torch.inference_mode():
        got = net(x.cuda(), t.cuda(), condition=text.cuda()).cpu()
        skipped = net(x.cuda(), t.cuda(), condition=text.cuda(), skip_layers=[0]).cpu()
    d, ds = _rel(got, ref.forward(x, t, text)), _rel(skipped, ref.forward(x, t, text, skip_layers=[0]))
    print("full forward vs oracle", shape_key, d, "skip_layers=[0]", ds)
    assert d < TOL and ds < TOL, (d, ds)
    assert _rel(skipped, got) > 5 * TOL  # (the skipped block is not a small one)


@pytest.mark.parametrize("cond", ["diff", "abs"])
def test_forward_with_r_against_oracle_and_its_mutants(cond):
    """tests/test_wan_full_ref.py holds every mutant at least 5 x TOL from the oracle for these seeds."""
    sd, x, t, r, text = W.r_case()
    net = _wan(sd, r_timestep=True, time_cond_type=cond)
    with torch.inference_mode():
        got = net(x.cuda(), t.cuda(), condition=text.cuda(), r=r.cuda()).cpu()
        plain = net(x.cuda(), t.cuda(), condition=text.cuda()).cpu()
    d = _rel(got, W.WanFullRef(sd, R.TINY, time_cond_type=cond).forward(x, t, text, r=r))
    dp = _rel(plain, W.WanFullRef(sd, R.TINY, time_cond_type=cond).forward(x, t, text))
    print("full forward with r vs oracle", cond, d, "without r", dp)
    assert d < TOL and dp < TOL, (d, dp)
    for m in W.MUTANTS:
        dm = _rel(got, W.WanFullRef(sd, R.TINY, time_cond_type=cond, mutant=m).forward(x, t, text, r=r))
        print("  mutant", m, dm)
        assert dm > d and dm > 5 * TOL, (m, dm, d)  # (the CPU test measures 0.38 ... 0.54 between each mutant and the oracle)


# ---- 3. a zero r_embedder ----------------------------------------------------------------------------------------------------------
def test_zero_r_embedder_with_r_is_the_call_without_r():
    sd = W.random_state_dict(R.TINY, 35, r_timestep=True, r_init="zero")
    x, t, text = _inputs("ragged", 36)
    net, without = _wan(sd, r_timestep=True), _wan(R.random_state_dict(R.TINY, 35))
    with torch.inference_mode():
        a = net(x.cuda(), t.cuda(), condition=text.cuda(), r=torch.tensor([0.3, 0.1], dtype=torch.float64).cuda())
        assert torch.isfinite(a).all() and torch.equal(a, net(x.cuda(), t.cuda(), condition=text.cuda()))
        assert torch.equal(a, without(x.cuda(), t.cuda(), condition=text.cuda()))  # ... and it is the network without the embedder


# ---- 4. the fused student loops ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", ["x0", "meanflow"])
def test_fused_loops_equal_the_generic_loops(loop, monkeypatch):
    """`FastGenModel.generator_fn(Wan)` / `MeanFlowModel.generator_fn(Wan(r_timestep=True))` take the fused loop (one
    fg_wan_full_sampler_run, one hipGraph); the same class's `_student_sample_loop` over `Wan.forward` is the per-step loop."""
    from fastgen_amd.methods.consistency_model.mean_flow import MeanFlowModel
    from fastgen_amd.methods.model import FastGenModel

    cls = FastGenModel if loop == "x0" else MeanFlowModel
    sd = W.random_state_dict(R.TINY, 37, r_timestep=loop == "meanflow")
    net = _wan(sd, r_timestep=loop == "meanflow")
    shp = W.SHAPES["ragged"]
    g = torch.Generator().manual_seed(38)
    noise, cond = torch.randn(shp, generator=g).cuda(), torch.randn(shp[0], 24, 128, generator=g).cuda()
    eps = torch.randn((2, *shp), generator=g).cuda()
    sch, gf = net.noise_scheduler, cls.generator_fn

    def per_step(steps, kind, t_list=None):
        tl = sch.get_t_list(steps, device="cuda") if t_list is None else torch.tensor(t_list, dtype=torch.float64, device="cuda")
        pending = [e for e in eps[: steps - 1]]
        monkeypatch.setattr(torch, "randn_like", lambda x, **kw: pending.pop(0))
        with torch.inference_mode():
            out = cls._student_sample_loop(net, sch.latents(noise, tl[0]), tl, condition=cond, student_sample_type=kind)
        monkeypatch.undo()
        return out

    kw = dict(student_sample_steps=3, condition=cond)
    captures, launches = _lib.graph_stats()
    for n, kind in enumerate(("sde", "ode")):
        want = per_step(3, kind)
        got = gf(net, noise, student_sample_type=kind, eps=eps, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, want), kind
        assert torch.equal(gf(net, noise, student_sample_type=kind, eps=eps, use_graph=False, **kw), want), kind
        assert _lib.graph_stats() == (captures + n + 1, launches + n + 1)  # one capture and launch per kind, none for the eager call
    # the cached graph replayed with another timestep list (same steps and zero pattern; `eps` is in the key by address)
    tl2 = [0.9, 0.6, 0.25, 0.0]
    captures, launches = _lib.graph_stats()
    got = gf(net, noise, student_sample_type="ode", eps=eps, t_list=tl2, **kw)
    assert _lib.graph_stats() == (captures, launches + 1), "the call with another timestep list captured a new graph"
    assert torch.equal(got, per_step(3, "ode", tl2))
    assert torch.equal(gf(net, noise, student_sample_steps=1, condition=cond), per_step(1, "sde"))
    # device draws: seed control
    a = gf(net, noise, seed=5, **kw)
    assert torch.equal(a, gf(net, noise, seed=5, **kw))
    assert not torch.equal(a, gf(net, noise, seed=6, **kw))
    with pytest.raises(_lib.FastGenAMDError):  # refused, not approximated
        gf(net, noise, student_sample_steps=1, t_list=[1.5, 0.0], condition=cond)
    # the 12-frame video: past total_num_frames, through the >= 1024-key attention path
    shp = W.SHAPES["long"]
    noise, cond = torch.randn(shp, generator=g).cuda(), torch.randn(shp[0], 24, 128, generator=g).cuda()
    assert torch.equal(gf(net, noise, student_sample_steps=2, condition=cond, student_sample_type="ode"), per_step(2, "ode"))


def test_student_loop_against_oracle():
    """Bound 3e-2: the project's bound for a 3-step student loop of this network against the fp32 oracle (tests/test_wan.py)."""
    from fastgen_amd.methods.model import FastGenModel

    sd = R.random_state_dict(R.TINY, 39)
    x, _, text = _inputs("ragged", 40)
    tl = [0.999, 0.6, 0.25, 0.0]
    want = W.x0_loop(W.WanFullRef(sd, R.TINY), x, torch.tensor(tl, dtype=torch.float64), text, sample_type="ode")
    got = FastGenModel.generator_fn(_wan(sd), x.cuda(), student_sample_steps=3, t_list=tl, condition=text.cuda(), student_sample_type="ode")
    print("x0 loop vs oracle", _rel(got.cpu(), want))
    assert _rel(got.cpu(), want) < 3e-2


# ---- 5. sample() -------------------------------------------------------------------------------------------------------------------
def _per_call_guided_loop(net, noise, cond, neg, guidance_scale, num_steps, shift, solver):
    """`Wan.sample` as separate calls: per solver step one `Wan.forward` of the stacked batch [x; x] against [cond; neg] (unguided: the
    plain batch) and the torch mirror of the update kernel (as tests/test_wan_guided.py::_per_call_guided_loop)."""
    guided = neg is not None and guidance_scale is not None
    B, sch = noise.shape[0], net.noise_scheduler
    text = torch.cat([cond, neg]) if guided else cond
    sig = solvers.flow_shift_sigmas(num_steps, shift)
    tab = solvers.multistep_table(sig, solver, guidance_scale if guided else 1.0)
    t_net = sch.safe_clamp(torch.floor(sig[:-1] * 1000.0) / 1000.0, min=sch.min_t, max=sch.max_t).cuda()
    stack = (lambda c: torch.cat([c, c])) if guided else (lambda c: c)
    cur, x_last, m_prev = sch.latents(noise, t_net[0]), None, None
    for i in range(num_steps):
        v = net(stack(cur), t_net[i].expand(text.shape[0]), condition=text, fwd_pred_type="flow")
        cur, x_last, m_prev = solvers.multistep_update(tab[i], cur, v[:B], x_last, m_prev, v_uncond=v[B:] if guided else None)
    return cur


@pytest.mark.parametrize("solver", ["unipc", "euler"])
def test_fused_guided_loop_equals_the_per_call_loop(solver):
    net, fresh = _wan(R.random_state_dict(R.TINY, 41)), _wan(R.random_state_dict(R.TINY, 41))
    shp = W.SHAPES["ragged"]
    g = torch.Generator().manual_seed(42)
    noise = torch.randn(shp, generator=g).cuda()
    cond, neg = torch.randn(shp[0], 16, 128, generator=g).cuda(), torch.randn(shp[0], 16, 128, generator=g).cuda()
    kw = dict(num_steps=3, solver=solver)
    with torch.inference_mode():
        want = _per_call_guided_loop(net, noise, cond, neg, 5.0, 3, 5.0, solver)
        keep = noise.clone()
        got = net.sample(noise, cond, neg, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, want) and torch.equal(noise, keep)
        captures, launches = _lib.graph_stats()
        assert torch.equal(net.sample(noise, cond, neg, **kw), want)  # replay of the one cached graph
        assert _lib.graph_stats() == (captures, launches + 1)
        assert torch.equal(net.sample(noise, cond, neg, use_graph=False, **kw), want)
        # the same graph with another table and guidance scale: device memory, nothing baked in
        want2 = _per_call_guided_loop(net, noise, cond, neg, 2.5, 3, 3.0, solver)
        assert not torch.equal(want2, want)
        assert torch.equal(net.sample(noise, cond, neg, guidance_scale=2.5, shift=3.0, **kw), want2)
        assert _lib.graph_stats() == (captures, launches + 2)
        # unguided: no negative condition (or no guidance scale), batch B
        want = _per_call_guided_loop(net, noise, cond, None, None, 3, 5.0, solver)
        assert torch.equal(net.sample(noise, cond, None, **kw), want)
        assert torch.equal(net.sample(noise, cond, neg, guidance_scale=None, use_graph=False, **kw), want)
        # a forward afterwards embeds its own text again
        t = torch.tensor([0.8, 0.45], dtype=torch.float64).cuda()
        assert torch.equal(net(noise, t, condition=cond), fresh(noise, t, condition=cond))


ORACLE_G, ORACLE_STEPS = 1.5, 4


@functools.lru_cache(maxsize=None)
def _oracle_case():
    """B = 1, 5 frames of 16 x 16, text [1, 16, 128] at scale 8 with the negative text its negation (tests/test_wan_guided.py's case)."""
    sd = R.random_state_dict(R.TINY, 41)
    g = torch.Generator().manual_seed(42)
    noise = torch.randn(1, 16, 5, 16, 16, generator=g)
    text = 8.0 * torch.randn(1, 16, 128, generator=g)
    return sd, noise, text, -text


@pytest.mark.parametrize("solver", ["unipc", "euler"])
def test_guided_loop_against_oracle(solver):
    """Bound: tests/test_wan_guided.py::test_guided_loop_against_oracle's - 3e-2 for a few-step loop of this network, the two flows'
    errors scaled by g and g - 1: (2 g - 1) x 3e-2 = 6e-2 at g = 1.5.  The oracle run with the two texts swapped must be further away."""
    sd, noise, text, neg = _oracle_case()
    ref = W.WanFullRef(sd, R.TINY)
    want = W.guided_sample(ref, noise, text, neg, ORACLE_G, ORACLE_STEPS, solver=solver)
    swapped = W.guided_sample(ref, noise, neg, text, ORACLE_G, ORACLE_STEPS, solver=solver)
    got = _wan(sd).sample(noise.cuda(), text.cuda(), neg.cuda(), guidance_scale=ORACLE_G, num_steps=ORACLE_STEPS, solver=solver).cpu()
    d, dsw = _rel(got, want), _rel(got, swapped)
    print("full guided loop vs oracle", solver, d, "swapped", dsw)
    assert d < (2 * ORACLE_G - 1) * 3e-2, d
    assert dsw > d, (d, dsw)


def test_hundred_steps():
    """The guided loop does not inherit the student loops' 64-step limit."""
    sd, noise, text, neg = _oracle_case()
    got = _wan(sd).sample(noise.cuda(), text.cuda(), neg.cuda(), guidance_scale=1.5, num_steps=100)
    assert torch.isfinite(got).all()


# ---- 6. the causal module beside it ------------------------------------------------------------------------------------------------
def test_causal_module_beside_the_bidirectional_calls():
    """The bidirectional entry points (a forward, a fused loop, a guided loop) between the two autoregressive calls of a CausalWan built
    beside the Wan module: the cache rows its first call stored are what its second call attends to, against its oracle."""
    from fastgen_amd.methods.model import FastGenModel

    sd = R.random_state_dict(R.TINY, 7)
    ref = R.CausalWanRef(sd, R.TINY)
    causal, net = _causal(sd, 6, chunk=2), _wan(sd)
    g = torch.Generator().manual_seed(8)
    B, H, W_ = 2, 16, 24
    x = torch.randn(B, 16, 5, H, W_, generator=g)
    text = torch.randn(B, 24, 128, generator=g)
    t = torch.tensor([0.6, 0.3], dtype=torch.float64)
    with torch.inference_mode():
        call = dict(condition=text.cuda(), fwd_pred_type="flow", is_ar=True)
        a0 = causal(x[:, :, :2].cuda(), torch.zeros(B, dtype=torch.float64).cuda(), cur_start_frame=0, store_kv=True, **call)
        net(x.cuda(), t.cuda(), condition=text.cuda())
        FastGenModel.generator_fn(net, x.cuda(), student_sample_steps=2, condition=text.cuda(), student_sample_type="ode")
        net.sample(x.cuda(), text.cuda(), -text.cuda(), num_steps=2)
        a1 = causal(x[:, :, 2:4].cuda(), t.cuda(), cur_start_frame=2, store_kv=False, **call)
    w0 = ref.forward(x[:, :, :2], torch.zeros(B, dtype=torch.float64), text, cur_start_frame=0, store_kv=True)
    w1 = ref.forward(x[:, :, 2:4], t, text, cur_start_frame=2, store_kv=False)
    assert _rel(a0.cpu(), w0) < TOL and _rel(a1.cpu(), w1) < TOL, (_rel(a0.cpu(), w0), _rel(a1.cpu(), w1))


# ---- 7. FSDP2 ------------------------------------------------------------------------------------------------------------------------
def test_fsdp2_one_rank_mesh_equals_bare_module():
    """`Wan.fully_shard` (Wan/network.py:761-782: every block, then the transformer - the r_embedder with it - as the root group) on a
    1-rank mesh, modelled on the CausalWan case of tests/test_gpu_dist.py.  Multi-rank: unmeasured."""
    import torch.distributed as dist
    from torch.distributed.device_mesh import init_device_mesh
    from torch.distributed.tensor import DTensor

    from fastgen_amd.methods.consistency_model.mean_flow import MeanFlowModel
    from fastgen_amd.networks import _weights

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
        sd = W.random_state_dict(R.TINY, 43, r_timestep=True)
        bare, net = _wan(sd, r_timestep=True), _wan(sd, r_timestep=True)
        net.fully_shard(mesh=mesh)
        assert all(isinstance(p, DTensor) for p in net.parameters())
        assert list(net.state_dict().keys()) == list(bare.state_dict().keys())
        groups = _weights.weight_groups(net, [n for n in net._names if "logvar" not in n])
        assert [g[0] for g in groups] == ["transformer.blocks.0.", "transformer.blocks.1.", "transformer."] and groups[2][1] == "transformer.blocks."
        x, t, text = _inputs("ragged", 44)
        x, t, text = x.cuda(), t.cuda(), text.cuda()
        r = torch.tensor([0.3, 0.1], dtype=torch.float64).cuda()
        with torch.inference_mode():
            assert torch.equal(net(x, t, condition=text, r=r), bare(x, t, condition=text, r=r))
            assert all(isinstance(p, DTensor) for p in net.parameters())
            kw = dict(student_sample_steps=2, t_list=[0.999, 0.5, 0.0], condition=text, student_sample_type="ode")
            assert torch.equal(MeanFlowModel.generator_fn(net, x, **kw), MeanFlowModel.generator_fn(bare, x, **kw))
            assert torch.equal(net.sample(x, text, -text, num_steps=2), bare.sample(x, text, -text, num_steps=2))
    finally:
        if created:
            dist.destroy_process_group()
