"""CausalWan: the second cache tag ("neg") and the guided teacher sampler `sample()` (fg_wan_select_cache_tag, fg_op_guided_multistep,
fg_wan_guided_sampler_run; reference fastgen/networks/Wan/network_causal.py:331-412, 1186-1295).  PARITY UNPINNED: the solver restates
diffusers' UniPC scheduler (fastgen_amd/networks/Wan/solvers.py); the tests hold the HIP path to that restatement and to the oracle.

CPU: the solver table (Euler identity, UniPC's order on a closed-form ODE, the sigma grid), the tag argument check, and the condition
under which the oracle comparison can tell a wrong guidance sign or scale from a right one.
GPU (-m gpu): the two tags as independent caches (bit-exact against two modules), tag "neg" against the oracle, the update kernel
against its torch mirror (bit-exact), the fused loop against the same loop made of separate calls (bit-exact), against the oracle, and
at 100 steps."""
import ctypes
import functools
import math

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd.networks.Wan import solvers
from oracle import wan_ref as R
import wan_guided_ref as G

KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2, chunk_size=2, total_num_frames=6)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _net(sd):
    from fastgen_amd.networks.Wan.network_causal import CausalWan

    net = CausalWan(**KW)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


# ---- CPU: the solver ------------------------------------------------------------------------------------------------------------
def test_euler_table_is_the_euler_step_exactly():
    g = torch.Generator().manual_seed(1)
    sig = solvers.flow_shift_sigmas(5, 3.0)
    tab = solvers.multistep_table(sig, "euler")
    assert tab.shape == (5, 8) and tab.dtype == torch.float64
    x, x_last, m_prev = torch.randn(3, 7, generator=g, dtype=torch.float64), None, None
    for i in range(5):
        v = torch.randn(3, 7, generator=g, dtype=torch.float64)
        want = x + (sig[i + 1] - sig[i]) * v
        x_next, x_corr, m = solvers.multistep_update(tab[i], x, v, x_last, m_prev)
        assert torch.equal(x_next, want), i
        assert torch.equal(x_corr, x), i  # the corrector is the identity
        x, x_last, m_prev = x_next, x_corr, m


def _gaussian_endpoint_error(n_steps, solver, s=4.0, x1=1.3):
    """|solver end point - closed form| for scalar Gaussian data of std s on the RF path x_t = (1 - t) x0 + t eps, with the exact
    predictor E[x0 | x_t] = (1 - t) s^2 x_t / ((1 - t)^2 s^2 + t^2).  The probability-flow ODE keeps x_t / std_t constant."""
    sig = solvers.flow_shift_sigmas(n_steps, 1.0)
    tab = solvers.multistep_table(sig, solver)
    var = lambda t: (1 - t) ** 2 * s * s + t * t
    x, x_last, m_prev = torch.tensor([x1], dtype=torch.float64), None, None
    for i in range(n_steps):
        t = float(sig[i])
        x0 = (1 - t) * s * s * x / var(t)
        x, x_last, m_prev = solvers.multistep_update(tab[i], x, (x - x0) / t, x_last, m_prev)
    return abs(float(x) - x1 * math.sqrt(var(0.0) / var(float(sig[0]))))


def test_unipc_is_second_order_and_euler_first_on_a_closed_form_ode():
    """N = 32 -> 64 steps, data std s = 4 (a smooth x0 predictor over the whole path: the asymptotic regime starts early; with s <= 1
    the UniPC error changes sign below N = 128 and single ratios mean nothing).  Closed form at these N: UniPC 4.3x, Euler 1.97x."""
    N = 32
    assert _gaussian_endpoint_error(N, "unipc") >= 3.0 * _gaussian_endpoint_error(2 * N, "unipc")
    assert _gaussian_endpoint_error(N, "euler") <= 2.5 * _gaussian_endpoint_error(2 * N, "euler")
    assert _gaussian_endpoint_error(2 * N, "unipc") < 0.1 * _gaussian_endpoint_error(2 * N, "euler")


def test_flow_shift_sigmas():
    for n, shift in [(1, 5.0), (3, 5.0), (50, 5.0), (100, 3.0)]:
        sig = solvers.flow_shift_sigmas(n, shift)
        assert sig.dtype == torch.float64 and sig.shape == (n + 1,)
        assert bool((sig[1:] < sig[:-1]).all()) and float(sig[-1]) == 0.0 and float(sig[0]) < 1.0
    n = 8
    want = torch.flip(1.0 - torch.linspace(1.0, 1.0 / 1000, n + 1, dtype=torch.float64), dims=(0,))
    assert torch.equal(solvers.flow_shift_sigmas(n, 1.0), want)  # shift = 1: the unshifted grid, 0.999 down to 0
    assert abs(float(solvers.flow_shift_sigmas(4, 5.0)[0]) - 5 * 0.999 / (1 + 4 * 0.999)) < 1e-15
    assert solvers.multistep_table(solvers.flow_shift_sigmas(100, 5.0), "unipc").isfinite().all()
    with pytest.raises(NotImplementedError):
        solvers.multistep_table(solvers.flow_shift_sigmas(4, 5.0), "dpm")


def test_select_cache_tag_rejects_other_tags():
    from fastgen_amd import _lib

    L = _lib.lib()
    cfg = _lib.fg_wan_config()
    cfg.num_heads, cfg.head_dim, cfg.in_channels, cfg.out_channels, cfg.text_dim, cfg.freq_dim = 2, 128, 16, 16, 128, 256
    cfg.ffn_dim, cfg.num_layers, cfg.rope_max_seq_len, cfg.chunk_size, cfg.total_num_frames, cfg.eps = 512, 2, 1024, 2, 6, 1e-6
    h = ctypes.c_void_p()
    if L.fg_wan_create(ctypes.byref(cfg), ctypes.byref(h)) != 0:
        pytest.skip("creating a handle needs a device here")
    try:
        FG_EINVAL = 1
        assert L.fg_wan_select_cache_tag(h, 2) == FG_EINVAL and b"tag" in L.fg_last_error()
        assert L.fg_wan_select_cache_tag(h, -1) == FG_EINVAL
        assert L.fg_wan_select_cache_tag(h, 1) == 0 and L.fg_wan_select_cache_tag(h, 1) == 0 and L.fg_wan_select_cache_tag(h, 0) == 0
        assert L.fg_wan_select_cache_tag(None, 0) == FG_EINVAL
    finally:
        L.fg_wan_destroy(h)


# ---- the oracle comparison's case: computed once, shared ------------------------------------------------------------------------------
ORACLE_G, ORACLE_STEPS, ORACLE_TOL = 1.5, 3, 6e-2  # tolerance (2 g - 1) * 3e-2: see test_guided_loop_against_oracle


@functools.lru_cache(maxsize=None)
def _oracle_case():
    """B = 1, 5 frames of 16 x 16, text [1, 16, 128] at scale 8 with the negative text its negation, weights of seed 41."""
    sd = R.random_state_dict(R.TINY, 41)
    g = torch.Generator().manual_seed(42)
    noise = torch.randn(1, 16, 5, 16, 16, generator=g)
    text = 8.0 * torch.randn(1, 16, 128, generator=g)
    return sd, noise, text, -text


@functools.lru_cache(maxsize=None)
def _oracle_sample(solver, guidance=ORACLE_G, swapped=False):
    sd, noise, text, neg = _oracle_case()
    pos_ref, neg_ref = G.two_tags(sd)
    a, b = (neg, text) if swapped else (text, neg)
    return G.guided_sample(pos_ref, neg_ref, noise, a, b, guidance, ORACLE_STEPS, solver=solver)


@pytest.mark.parametrize("solver", ["unipc", "euler"])
def test_oracle_case_separates_a_wrong_guidance_from_a_right_one(solver):
    """The bound of the GPU comparison must not hide a wrong guidance: without guidance (g = 1) and with the two texts swapped the
    oracle's own output moves by more than 4 x the bound (measured: 0.25 and 1.0)."""
    true = _oracle_sample(solver)
    assert _rel(_oracle_sample(solver, guidance=1.0), true) > 4 * ORACLE_TOL
    assert _rel(_oracle_sample(solver, swapped=True), true) > 4 * ORACLE_TOL


# ---- GPU: the cache tags -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tags_are_independent_caches():
    sd = R.random_state_dict(R.TINY, 51)
    net, one, two = _net(sd), _net(sd), _net(sd)
    g = torch.Generator().manual_seed(52)
    x = torch.randn(1, 16, 5, 16, 16, generator=g).cuda()
    texts = {"pos": torch.randn(1, 16, 128, generator=g).cuda(), "neg": torch.randn(1, 16, 128, generator=g).cuda()}
    alone = {"pos": one, "neg": two}
    calls = [("pos", 0, 3, 0.0, True), ("neg", 0, 3, 0.0, True), ("pos", 3, 5, 0.6, False), ("neg", 3, 5, 0.6, False)]
    fresh = _net(sd)

    def run(module, tag, module_tag, lo, hi, t, store):
        tt = torch.full((1,), t, dtype=torch.float64, device="cuda")
        return module(x[:, :, lo:hi], tt, condition=texts[tag], fwd_pred_type="flow", cache_tag=module_tag, cur_start_frame=lo, store_kv=store,
                      is_ar=True)

    with torch.inference_mode():
        want = [run(alone[tag], tag, "pos", lo, hi, t, store) for (tag, lo, hi, t, store) in calls]
        assert not torch.equal(want[2], want[3])  # (the two texts do give different outputs)
        for _ in range(2):  # ... and again after clear_caches(), which resets both tags
            got = [run(net, tag, tag, lo, hi, t, store) for (tag, lo, hi, t, store) in calls]
            for a, b in zip(got, want):
                assert torch.isfinite(a).all() and torch.equal(a, b)
            net.clear_caches()
        # nothing stored under "neg" (only under "pos"): a "neg" call behind frame 0 is the same call on a fresh module
        run(net, "pos", "pos", 0, 3, 0.0, True)
        got = run(net, "neg", "neg", 3, 5, 0.6, False)
        assert torch.equal(got, run(fresh, "neg", "pos", 3, 5, 0.6, False))
        assert not torch.equal(got, want[3])
        with pytest.raises(NotImplementedError, match="'pos' and 'neg'"):
            run(net, "pos", "other", 0, 3, 0.0, False)
        net.clear_caches()


@pytest.mark.gpu
def test_tag_neg_calls_against_oracle():
    """The call sequence of test_wan.py::test_autoregressive_calls_against_oracle under cache_tag="neg", same bound."""
    sd = R.random_state_dict(R.TINY, 7)
    ref, net = R.CausalWanRef(sd, R.TINY), _net(sd)
    g = torch.Generator().manual_seed(8)
    B, H, W = 2, 16, 24
    x = torch.randn(B, 16, 4, H, W, generator=g)
    text = torch.randn(B, 40, 128, generator=g)
    with torch.inference_mode():
        for (lo, hi, t, store) in [(0, 2, 0.8, False), (0, 2, 0.0, True), (2, 4, 0.6, False), (2, 4, 0.0, True)]:
            tt = torch.full((B,), t, dtype=torch.float64)
            want = ref.forward(x[:, :, lo:hi], tt, text, cur_start_frame=lo, store_kv=store)
            got = net(x[:, :, lo:hi].cuda(), tt.cuda(), condition=text.cuda(), fwd_pred_type="flow", cache_tag="neg", cur_start_frame=lo,
                      store_kv=store, is_ar=True)
            assert got.shape == want.shape
            print("tag neg vs oracle", lo, t, store, _rel(got.cpu(), want))
            assert _rel(got.cpu(), want) < 2e-2, (lo, t, store, _rel(got.cpu(), want))
        net.clear_caches()


# ---- GPU: the update kernel ------------------------------------------------------------------------------------------------------------
def _op_multistep(v, x, x_last, m_prev, row, guided, first, with_x2):
    from fastgen_amd import _lib

    total = x.numel()
    x, x_last, m_prev = x.clone(), x_last.clone(), m_prev.clone()
    x2 = torch.full_like(x, float("nan")) if with_x2 else None
    tab = row.to(torch.float64).cuda().contiguous()
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    _lib.check(_lib.lib().fg_op_guided_multistep(p(v), p(x), p(x2), p(x_last), p(m_prev), p(tab), int(guided), int(first), total,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return x, x2, x_last, m_prev


@pytest.mark.gpu
@pytest.mark.parametrize("total", [1, 7, 4097, 2 * 1026, 65536 + 4])  # 2 x 1026: two rows that are no multiple of the 4-wide access
def test_update_kernel_equals_its_torch_mirror(total):
    g = torch.Generator().manual_seed(total)
    tab = solvers.multistep_table(solvers.flow_shift_sigmas(3, 5.0), "unipc", 1.5)
    for guided in (True, False):
        for step in (0, 1, 2):  # step 0: no history, x_last / m_prev (NaN here) must not be read
            first = step == 0
            v = torch.randn(2 * total if guided else total, generator=g).cuda()
            x = torch.randn(total, generator=g).cuda()
            x_last, m_prev = torch.randn(total, generator=g).cuda(), torch.randn(total, generator=g).cuda()
            if first:
                x_last, m_prev = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
            want = solvers.multistep_update(tab[step], x, v[:total], None if first else x_last, None if first else m_prev,
                                            v_uncond=v[total:] if guided else None)
            for with_x2 in (True, False):
                got_x, got_x2, got_last, got_m = _op_multistep(v, x, x_last, m_prev, tab[step], guided, first, with_x2)
                assert torch.isfinite(got_x).all()
                assert torch.equal(got_x, want[0]) and torch.equal(got_last, want[1]) and torch.equal(got_m, want[2]), (guided, step)
                assert got_x2 is None or torch.equal(got_x2, want[0])


# ---- GPU: the fused loop ---------------------------------------------------------------------------------------------------------------
def _per_call_guided_loop(net, x, cond, neg, guidance_scale, sample_steps, shift, solver, context_noise=0.0, eps=None):
    """`CausalWan.sample` as separate calls: per solver step one `CausalWan.forward` of the stacked batch [x; x] against [cond; neg]
    (unguided: the plain batch) and the torch mirror of the update kernel, then the cache-fill call."""
    guided = neg is not None
    B, F, cs, sch = x.shape[0], x.shape[2], net.chunk_size, net.noise_scheduler
    text = torch.cat([cond, neg]) if guided else cond
    sig = solvers.flow_shift_sigmas(sample_steps, shift)
    tab = solvers.multistep_table(sig, solver, guidance_scale if guided else 1.0)
    t_net = (torch.floor(sig[:-1] * 1000.0) / 1000.0).cuda()
    stack = (lambda c: torch.cat([c, c])) if guided else (lambda c: c)
    n, rem = F // cs, F % cs
    bounds = [(0, rem)] if n == 0 else [(0 if i == 0 else cs * i + rem, cs * (i + 1) + rem) for i in range(n)]
    call = dict(condition=text, fwd_pred_type="flow", is_ar=True)
    net.clear_caches()
    for a, b in bounds:
        cur, x_last, m_prev = x[:, :, a:b], None, None
        for i in range(sample_steps):
            v = net(stack(cur), t_net[i].expand(text.shape[0]), cur_start_frame=a, store_kv=False, **call)
            cur, x_last, m_prev = solvers.multistep_update(tab[i], cur, v[:B], x_last, m_prev, v_uncond=v[B:] if guided else None)
        x[:, :, a:b] = cur
        tc, xc = torch.zeros(text.shape[0], dtype=torch.float64, device="cuda"), cur
        if context_noise > 0:
            tc = torch.full((text.shape[0],), context_noise, device=x.device, dtype=x.dtype)
            xc = sch.forward_process(cur, eps[:, :, a:b], tc[:B])
        net(stack(xc), tc, cur_start_frame=a, store_kv=True, **call)
    net.clear_caches()
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["unipc", "euler"])
def test_fused_guided_loop_equals_the_per_call_loop(solver):
    net = _net(R.random_state_dict(R.TINY, 23))
    g = torch.Generator().manual_seed(24)
    B, F, H, W = 2, 5, 16, 24
    noise = torch.randn(B, 16, F, H, W, generator=g).cuda()
    cond, neg = torch.randn(B, 16, 128, generator=g).cuda(), torch.randn(B, 16, 128, generator=g).cuda()
    eps = torch.randn(B, 16, F, H, W, generator=g).cuda()
    kw = dict(sample_steps=3, solver=solver)
    with torch.inference_mode():
        want = _per_call_guided_loop(net, noise.clone(), cond, neg, 5.0, 3, 5.0, solver)
        got = net.sample(noise.clone(), cond, neg, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, want)
        captures, launches = _lib.graph_stats()
        assert torch.equal(net.sample(noise.clone(), cond, neg, **kw), want)  # replay of the cached chunk graphs
        assert _lib.graph_stats() == (captures, launches + 2)
        assert torch.equal(net.sample(noise.clone(), cond, neg, use_graph=False, **kw), want)
        # the same graphs with another table and guidance scale: device memory, nothing baked in
        want2 = _per_call_guided_loop(net, noise.clone(), cond, neg, 2.5, 3, 3.0, solver)
        assert not torch.equal(want2, want)
        assert torch.equal(net.sample(noise.clone(), cond, neg, guidance_scale=2.5, shift=3.0, **kw), want2)
        assert _lib.graph_stats() == (captures, launches + 4)
        # the cache-fill call on the re-noised chunk, injected noise
        want = _per_call_guided_loop(net, noise.clone(), cond, neg, 5.0, 3, 5.0, solver, context_noise=0.1, eps=eps)
        assert torch.equal(net.sample(noise.clone(), cond, neg, context_noise=0.1, eps=eps, **kw), want)
        assert torch.equal(net.sample(noise.clone(), cond, neg, context_noise=0.1, eps=eps, use_graph=False, **kw), want)
        # device draws: seed control
        a = net.sample(noise.clone(), cond, neg, context_noise=0.1, seed=3, **kw)
        assert torch.equal(a, net.sample(noise.clone(), cond, neg, context_noise=0.1, seed=3, **kw))
        assert not torch.equal(a, net.sample(noise.clone(), cond, neg, context_noise=0.1, seed=4, **kw))
        # unguided: no negative condition (or no guidance scale), batch B
        want = _per_call_guided_loop(net, noise.clone(), cond, None, None, 3, 5.0, solver)
        assert torch.equal(net.sample(noise.clone(), cond, None, **kw), want)
        assert torch.equal(net.sample(noise.clone(), cond, neg, guidance_scale=None, use_graph=False, **kw), want)
        # the per-call entry points still work afterwards, under both tags
        t0 = torch.full((B,), 0.5, dtype=torch.float64, device="cuda")
        for tag in ("pos", "neg"):
            assert torch.isfinite(net(noise[:, :, :3], t0, condition=cond, cache_tag=tag, cur_start_frame=0, store_kv=True, is_ar=True)).all()
        net.clear_caches()


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["unipc", "euler"])
def test_guided_loop_against_oracle(solver):
    """Bound: 3e-2 is the project's bound for the 3-step student loop on this shape (bf16 network against the fp32 oracle); guidance
    v_u + g (v_c - v_u) scales the two flows' errors by g and g - 1: (2 g - 1) x 3e-2 = 6e-2 at g = 1.5.
    test_oracle_case_separates_a_wrong_guidance_from_a_right_one holds the case to a separation of 4 x that."""
    sd, noise, text, neg = _oracle_case()
    net = _net(sd)
    want = _oracle_sample(solver)
    got = net.sample(noise.clone().cuda(), text.cuda(), neg.cuda(), guidance_scale=ORACLE_G, sample_steps=ORACLE_STEPS, solver=solver)
    assert got.shape == want.shape
    print("guided loop vs oracle", solver, _rel(got.cpu(), want))
    assert _rel(got.cpu(), want) < (2 * ORACLE_G - 1) * 3e-2, _rel(got.cpu(), want)


@pytest.mark.gpu
def test_hundred_steps():
    """The guided loop does not inherit the student loops' 64-step limit."""
    sd, noise, text, neg = _oracle_case()
    net = _net(sd)
    got = net.sample(noise.clone().cuda(), text.cuda(), neg.cuda(), guidance_scale=1.5, sample_steps=100)
    assert torch.isfinite(got).all()
    assert torch.equal(got, net.sample(noise.clone().cuda(), text.cuda(), neg.cuda(), guidance_scale=1.5, sample_steps=100, use_graph=False))
