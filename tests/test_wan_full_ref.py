"""The bidirectional video DiT `Wan` (fastgen_amd/networks/Wan/network.py; fg_wan_create_ex, fg_wan_forward_full), what a machine
without a GPU can hold: the oracle tests/wan_full_ref.py against the causal oracle it is composed from, its r term (zero embedder,
"diff" against "abs"), that its mutants - the mistakes the GPU comparison has to catch - stand far enough from it, the module's state
dict and r_embedder inits, the C ABI's parameter table and host-side refusals, and the module's refusals; for the per-block pin
tests/test_gpu_wan_full_blocks.py: the launch plan of every case, the distance of its mutants (m) - (q) from the oracle, and the
refusals of fg_wan_forward_full_features.  PARITY UNPINNED."""
import ctypes
import functools

import pytest
import torch

from oracle import wan_ref as R
import wan_full_ref as W

KW = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2)
FG_EINVAL, FG_ENOTREADY = 1, 2


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---- 1. the oracle against the oracle it is composed from -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_forward_is_the_block_causal_oracle_with_one_chunk(dtype):
    """A block-wise causal mask whose one chunk holds every frame masks nothing."""
    sd = R.random_state_dict(R.TINY, 3)
    g = torch.Generator().manual_seed(4)
    B, Fr = 2, 4
    x = torch.randn(B, 16, Fr, 8, 12, generator=g)
    text = torch.randn(B, 9, 128, generator=g)
    t = torch.tensor([0.7, 0.2], dtype=torch.float64)
    cfg = R.WanConfig(num_heads=2, head_dim=128, text_dim=128, ffn_dim=512, num_layers=2, chunk_size=Fr + 1, total_num_frames=Fr)
    want = R.CausalWanRef(sd, cfg, dtype).forward(x, t, text, block_causal=True)
    got = W.WanFullRef(sd, R.TINY, dtype).forward(x, t, text)
    if dtype == torch.float64:
        assert torch.equal(got, want)
    else:
        assert torch.allclose(got, want, atol=1e-6, rtol=0)
    # skip_layers: passing over every block leaves the patch embedding under the output layer; over one block, something else
    ref = W.WanFullRef(sd, R.TINY, dtype)
    none = ref.forward(x, t, text, skip_layers=[0, 1])
    assert _rel(ref.forward(x, t, text, skip_layers=[0]), got) > 0.1 and _rel(none, got) > 0.1
    p = ref.p
    assert torch.equal(none, R.final_layer(p, R.TINY, R.patch_embed(p, x.to(dtype)),
                                           R.time_embedding(p, R.TINY, (1000.0 * t.float()).view(B, 1).expand(B, Fr).reshape(-1).to(dtype)), Fr, 4, 6))


# ---- 2. / 3. the r term -----------------------------------------------------------------------------------------------------------
def _small_r_inputs():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 16, 3, 8, 12, generator=g)
    text = torch.randn(2, 9, 128, generator=g)
    return x, torch.tensor([0.7, 0.2], dtype=torch.float64), torch.tensor([0.4, 0.05], dtype=torch.float64), text


def test_oracle_zero_r_embedder_is_no_r_embedder():
    x, t, r, text = _small_r_inputs()
    ref = W.WanFullRef(W.random_state_dict(R.TINY, 5, r_timestep=True, r_init="zero"), R.TINY)
    assert torch.equal(ref.forward(x, t, text, r=r), ref.forward(x, t, text))
    with pytest.raises(ValueError, match="no r_embedder"):  # (the reference's, Wan/network.py:356)
        W.WanFullRef(R.random_state_dict(R.TINY, 5), R.TINY).forward(x, t, text, r=r)


def test_oracle_diff_at_r_zero_is_abs_at_r_equal_t():
    """The embedder sees fp32(1000 t) - fp32(0) on one side and fp32(1000 t) on the other: the same number, so the same output."""
    x, t, _, text = _small_r_inputs()
    sd = W.random_state_dict(R.TINY, 5, r_timestep=True)
    diff = W.WanFullRef(sd, R.TINY, time_cond_type="diff").forward(x, t, text, r=torch.zeros_like(t))
    abs_ = W.WanFullRef(sd, R.TINY, time_cond_type="abs").forward(x, t, text, r=t)
    assert torch.equal(diff, abs_)
    assert _rel(W.WanFullRef(sd, R.TINY).forward(x, t, text), diff) > 0.1  # (and the r term is not a small one)


def test_oracle_loops_of_one_step():
    """One step to t = 0: both student loops are noise * t_0 - t_0 * flow (MeanFlow: r = 0 in 'sde' and in 'ode' alike), and the
    unguided teacher loop with the Euler table is the same step from sigma_0."""
    x, _, _, text = _small_r_inputs()
    sd = W.random_state_dict(R.TINY, 5, r_timestep=True)
    ref = W.WanFullRef(sd, R.TINY, torch.float64)
    tl = torch.tensor([0.9, 0.0], dtype=torch.float64)
    xt = x.double() * 0.9
    want = xt - 0.9 * ref.forward(xt, tl[0].expand(2), text)
    assert torch.equal(W.x0_loop(ref, x.double(), tl, text), want)
    want_r = xt - 0.9 * ref.forward(xt, tl[0].expand(2), text, r=torch.zeros(2, dtype=torch.float64))
    for kind in ("sde", "ode"):
        assert torch.allclose(W.meanflow_loop(ref, x.double(), tl, text, sample_type=kind), want_r, rtol=0, atol=1e-12)
    assert _rel(want_r, want) > 0.1
    s0 = 0.999  # flow_shift_sigmas(1, .): sigma_0 = shift * 0.999 / (1 + (shift - 1) * 0.999), shift = 1
    x1 = x.double() * s0
    got = W.guided_sample(ref, x, text, None, None, 1, shift=1.0, solver="euler")
    assert torch.allclose(got, x1 - s0 * ref.forward(x1, torch.full((2,), s0, dtype=torch.float64), text), rtol=0, atol=1e-12)


# ---- 4. the mutants of the GPU comparison -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _r_outputs(cond):
    sd, x, t, r, text = W.r_case()
    right = W.WanFullRef(sd, R.TINY, time_cond_type=cond).forward(x, t, text, r=r)
    return right, {m: W.WanFullRef(sd, R.TINY, time_cond_type=cond, mutant=m).forward(x, t, text, r=r) for m in W.MUTANTS}


@pytest.mark.parametrize("cond", ["diff", "abs"])
def test_oracle_mutants_stand_apart_from_the_oracle(cond):
    """The GPU test holds the HIP path to rel-L2 < 2e-2 of the oracle.  Each wrong r term - ignored, the other time_cond_type,
    r_timestep_proj without remb - is at least 5 x that bound away at the GPU test's seeds: the r_embedder's weights are drawn at the
    t embedder's scale (`random_state_dict(r_timestep=True)`) for exactly this."""
    right, mutants = _r_outputs(cond)
    for name, out in mutants.items():
        d = _rel(out, right)
        print("mutant", cond, name, d)
        assert d >= 0.1, (cond, name, d)


# ---- 5. the module's state dict ---------------------------------------------------------------------------------------------------
def _wan(**kw):
    from fastgen_amd.networks.Wan.network import Wan

    return Wan(**dict(KW, **kw))


def test_module_state_dict():
    plain = _wan().state_dict()
    want = R.state_dict_shapes(R.TINY)
    assert list(plain) == list(want) and all(tuple(plain[k].shape) == v for k, v in want.items())
    with_r = _wan(r_timestep=True).state_dict()
    want_r = W.state_dict_shapes(R.TINY, r_timestep=True)
    assert list(with_r) == list(want_r) and all(tuple(with_r[k].shape) == v for k, v in want_r.items())
    assert list(with_r)[-6:] == ["transformer.r_embedder." + k for k in W.R_KEYS]
    assert list(with_r)[: len(plain)] == list(plain) and all(torch.equal(with_r[k], plain[k]) for k in plain)
    assert list(_wan(enable_logvar_linear=False).state_dict()) == [k for k in want if "logvar_linear" not in k]
    # the oracle's state dicts load
    _wan().load_state_dict(R.random_state_dict(R.TINY, 1), strict=True)
    _wan(r_timestep=True).load_state_dict(W.random_state_dict(R.TINY, 1, r_timestep=True), strict=True)


def test_r_embedder_inits():
    """`init_embedder` (Wan/network.py:808-831): "pretrained" is the condition_embedder's copy, "zero" all zeros, "random" leaves
    time_embedder.linear_2 and time_proj at zero (remb and r_timestep_proj start at zero) and the biases at zero."""
    ce, re = "transformer.condition_embedder.", "transformer.r_embedder."
    sd = _wan(r_timestep=True, r_embedder_init="pretrained").state_dict()
    assert all(torch.equal(sd[re + k], sd[ce + k]) for k in W.R_KEYS)
    assert torch.equal(_wan(r_timestep=True).state_dict()[re + W.R_KEYS[0]], sd[re + W.R_KEYS[0]])  # the default
    sd = _wan(r_timestep=True, r_embedder_init="zero").state_dict()
    assert all(not sd[re + k].any() for k in W.R_KEYS)
    sd = _wan(r_timestep=True, r_embedder_init="random").state_dict()
    assert all(not sd[re + k].any() for k in W.R_KEYS[1:])
    w = sd[re + W.R_KEYS[0]]
    assert w.any() and abs(float(w.std()) - 0.02) < 2e-3 and not torch.equal(w, sd[ce + W.R_KEYS[0]])
    net = _wan(r_timestep=True, r_embedder_init="zero")
    net.init_r_embedder("pretrained")  # (after a checkpoint without the r_embedder was loaded)
    sd = net.state_dict()
    assert all(torch.equal(sd[re + k], sd[ce + k]) for k in W.R_KEYS)
    with pytest.raises(ValueError, match="Invalid embedder_init"):
        _wan(r_timestep=True, r_embedder_init="ones")
    with pytest.raises(ValueError, match="Invalid time condition"):
        _wan(r_timestep=True, time_cond_type="rel")


# ---- 6. the C ABI -----------------------------------------------------------------------------------------------------------------
def _abi_cfg():
    from fastgen_amd import _lib

    cfg = _lib.fg_wan_config()
    cfg.num_heads, cfg.head_dim, cfg.in_channels, cfg.out_channels, cfg.text_dim, cfg.freq_dim = 2, 128, 16, 16, 128, 256
    cfg.ffn_dim, cfg.num_layers, cfg.rope_max_seq_len, cfg.chunk_size, cfg.total_num_frames, cfg.eps = 512, 2, 1024, 2, 6, 1e-6
    return cfg


def _table(L, h):
    name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 5)()
    out = []
    for i in range(L.fg_wan_num_params(h)):
        assert L.fg_wan_param_info(h, i, ctypes.byref(name), ctypes.byref(ndim), shape) == 0
        out.append((name.value.decode(), tuple(shape[j] for j in range(ndim.value))))
    return out


def test_abi_create_ex_and_forward_full_refusals():
    """Host-only calls: no device memory is touched (the pointers handed in are never dereferenced)."""
    from fastgen_amd import _lib

    L = _lib.lib()
    assert ctypes.sizeof(_lib.fg_wan_config) == 13 * 4 and ctypes.sizeof(_lib.fg_wan_ext_config) == 2 * 4
    made = []

    def create(ext):
        h = ctypes.c_void_p()
        rc = L.fg_wan_create_ex(ctypes.byref(_abi_cfg()), ctypes.byref(ext) if ext is not None else None, ctypes.byref(h))
        if rc == 0:
            made.append(h)
        return rc, h

    def ext(r, diff):
        e = _lib.fg_wan_ext_config()
        e.r_timestep, e.time_cond_diff = r, diff
        return e

    try:
        h0 = ctypes.c_void_p()
        assert L.fg_wan_create(ctypes.byref(_abi_cfg()), ctypes.byref(h0)) == 0
        made.append(h0)
        base = _table(L, h0)
        assert dict(base) == R.state_dict_shapes(R.TINY) and [n for n, _ in base] == list(R.state_dict_shapes(R.TINY))
        for e in (None, ext(0, 0)):
            rc, h = create(e)
            assert rc == 0 and _table(L, h) == base
        rc, hr = create(ext(1, 1))
        assert rc == 0
        tab = _table(L, hr)
        want = W.state_dict_shapes(R.TINY, r_timestep=True)
        assert tab[: len(base)] == base and [n for n, _ in tab[len(base):]] == ["transformer.r_embedder." + k for k in W.R_KEYS]
        assert dict(tab) == want
        for bad in (ext(2, 0), ext(0, -1)):
            rc, h = create(bad)
            assert rc == FG_EINVAL and not h.value

        fake = ctypes.c_void_p(4096)  # non-null, 256-byte aligned, never dereferenced
        sk = lambda *v: (ctypes.c_int * len(v))(*v)

        def full(h, r, skip, n):
            return L.fg_wan_forward_full(h, fake, fake, r, ctypes.c_void_p(8192), 1, 2, 16, 16, skip, n, fake, 1 << 30, None)

        assert full(h0, fake, None, 0) == FG_EINVAL and b"r_embedder" in L.fg_last_error()
        for skip in (sk(1, 0), sk(0, 0), sk(2), sk(-1)):
            assert full(hr, None, skip, len(skip)) == FG_EINVAL and b"skip_layers" in L.fg_last_error(), list(skip)
        assert full(hr, None, None, 1) == FG_EINVAL
        # well-formed arguments on a handle whose weights were never packed
        assert full(hr, fake, sk(0, 1), 2) == FG_ENOTREADY and b"not packed" in L.fg_last_error()
        assert full(h0, None, None, 0) == FG_ENOTREADY

        # fg_wan_forward_full_features: fg_wan_forward_features' tap checks, fg_wan_forward_full's, and a block in both lists
        taps2 = (_lib.fg_wan_block_taps * 2)()

        def feat(h, r=None, skip=None, n=0, blocks=sk(0, 1), taps=taps2, nt=2, frames=2):
            return L.fg_wan_forward_full_features(h, fake, fake, r, ctypes.c_void_p(8192), 1, frames, 16, 16, skip, n, blocks, taps, nt, None, None,
                                                  None, fake, 1 << 30, None)

        assert feat(hr, skip=sk(1), n=1) == FG_EINVAL and b"both tapped and in skip_layers" in L.fg_last_error()
        assert feat(hr, skip=sk(0, 1), n=2, blocks=sk(1), nt=1) == FG_EINVAL and b"both tapped" in L.fg_last_error()
        assert feat(h0, r=fake) == FG_EINVAL and b"r_embedder" in L.fg_last_error()
        for blocks in (sk(1, 0), sk(0, 0), sk(0, 2), sk(-1, 0)):
            assert feat(hr, blocks=blocks) == FG_EINVAL and b"tap_blocks" in L.fg_last_error(), list(blocks)
        assert feat(hr, blocks=None) == FG_EINVAL and feat(hr, taps=None) == FG_EINVAL and feat(hr, nt=-1) == FG_EINVAL
        assert feat(hr, skip=sk(1, 1), n=2, blocks=sk(0), nt=1) == FG_EINVAL and b"skip_layers must be ascending" in L.fg_last_error()
        # frames beyond the RoPE table (rope_max_seq_len = 1024): refused by both full calls from the arguments alone
        assert feat(hr, frames=1025) == FG_EINVAL and b"RoPE table" in L.fg_last_error() and feat(hr, frames=1024) == FG_ENOTREADY
        assert L.fg_wan_forward_full(hr, fake, fake, None, ctypes.c_void_p(8192), 1, 1025, 16, 16, None, 0, fake, 1 << 30, None) == FG_EINVAL
        assert b"RoPE table" in L.fg_last_error()
        assert L.fg_wan_forward_full_features(None, fake, fake, None, fake, 1, 2, 16, 16, None, 0, None, None, 0, None, None, None, fake, 1 << 30,
                                              None) == FG_EINVAL
        # well-formed (one block skipped, the other tapped; no taps at all) on handles that were never packed
        assert feat(hr, r=fake, skip=sk(0), n=1, blocks=sk(1), nt=1) == FG_ENOTREADY and b"not packed" in L.fg_last_error()
        assert feat(h0, blocks=None, taps=None, nt=0) == FG_ENOTREADY
        # workspace sizes: any frame count (the cap of total_num_frames = 6 is the causal calls'), 0 for a bad shape
        assert L.fg_wan_full_workspace_bytes(hr, 1, 12, 16, 24) > L.fg_wan_full_workspace_bytes(hr, 1, 5, 16, 24) > 0
        assert L.fg_wan_full_workspace_bytes(hr, 1, 5, 15, 24) == 0
        assert L.fg_wan_full_sampler_workspace_bytes(hr, 2, 12, 16, 24) > 0 and L.fg_wan_full_sampler_workspace_bytes(hr, 2, 1025, 16, 24) == 0
        assert L.fg_wan_full_guided_sampler_workspace_bytes(hr, 2, 12, 16, 24, 100, 1) > L.fg_wan_full_guided_sampler_workspace_bytes(hr, 2, 12, 16, 24, 100, 0)
        # the loops' argument checks come before the handle's state
        sc = _lib.fg_wan_sampler_config()
        sc.t_scale, sc.net_pred_flow, sc.schedule = 1000.0, 1, _lib.FG_SCHEDULE_RF
        tl = (ctypes.c_double * 3)(0.9, 0.5, 0.0)

        def loop(h, kind, **kw):
            c = _lib.fg_wan_sampler_config.from_buffer_copy(sc)
            for k, v in kw.items():
                setattr(c, k, v)
            return L.fg_wan_full_sampler_run(h, ctypes.byref(c), fake, tl, 2, _lib.FG_SAMPLE_ODE, kind, None, 0, ctypes.c_void_p(8192), 1, 2, 16, 16,
                                             fake, 1 << 40, 0, None)

        assert loop(h0, _lib.FG_LOOP_MEANFLOW) == FG_EINVAL and b"r_embedder" in L.fg_last_error()
        assert loop(hr, _lib.FG_LOOP_MEANFLOW, net_pred_flow=0) == FG_EINVAL
        assert loop(hr, _lib.FG_LOOP_EULER) == FG_EINVAL
        assert loop(hr, _lib.FG_LOOP_X0, context_noise=0.1) == FG_EINVAL and b"context_noise" in L.fg_last_error()
        assert loop(hr, _lib.FG_LOOP_X0, prefill_frames=2) == FG_EINVAL
        assert loop(hr, _lib.FG_LOOP_MEANFLOW) == FG_ENOTREADY and loop(h0, _lib.FG_LOOP_X0) == FG_ENOTREADY
    finally:
        for h in made:
            L.fg_wan_destroy(h)


# ---- 7. the module's refusals -----------------------------------------------------------------------------------------------------
def test_module_refusals():
    from fastgen_amd.networks.Wan.network_causal import CausalWan

    with pytest.raises(NotImplementedError, match="norm_temb"):
        _wan(norm_temb=True)
    with pytest.raises(NotImplementedError, match="encoder_depth"):
        _wan(encoder_depth=1)
    with pytest.raises(ValueError, match="compute_dtype"):
        _wan(compute_dtype="fp16")
    with pytest.raises(ValueError, match="multiple of 128"):
        _wan(compute_dtype="fp8", ffn_dim=576)
    _wan(norm_temb=False, encoder_depth=None, load_pretrained=False, model_id_or_local_path="Wan-AI/Wan2.1-T2V-1.3B-Diffusers")
    x, t, r, text = _small_r_inputs()
    net, net_r = _wan(), _wan(r_timestep=True)
    with torch.no_grad():
        with pytest.raises(ValueError, match="no r_embedder is present"):
            net(x, t, condition=text, r=r)
        for kw in (dict(feature_indices={0}), dict(return_features_early=True), dict(return_logvar=True)):
            with pytest.raises(NotImplementedError, match="feature taps / logvar"):
                net(x, t, condition=text, **kw)
        with pytest.raises(TypeError, match="unexpected forward kwargs"):
            net(x, t, condition=text, is_ar=False)
        for n, kw in ((net, {}), (net_r, dict(r=r)), (net, dict(skip_layers=[0]))):
            with pytest.raises(RuntimeError, match="HIP GPU only"):
                n(x, t, condition=text, **kw)
        with pytest.raises(RuntimeError, match="HIP GPU only"):
            net.few_step_sample(x, text, [0.9, 0.0])
        with pytest.raises(RuntimeError, match="HIP GPU only"):
            net.sample(x, text, -text, num_steps=2)
        with pytest.raises(NotImplementedError, match="skip_layers in sample"):
            net.sample(x, text, -text, num_steps=2, skip_layers=[0])
        with pytest.raises(NotImplementedError, match="no loop 'meanflow'"):
            net.few_step_sample(x, text, [0.9, 0.0], loop="meanflow")
    assert net.supports_fused_loop("x0") and not net.supports_fused_loop("meanflow") and not net.supports_fused_loop("euler")
    assert net_r.supports_fused_loop("x0") and net_r.supports_fused_loop("meanflow")
    assert not _wan(r_timestep=True, net_pred_type="x0").supports_fused_loop("meanflow")
    with pytest.raises(NotImplementedError, match="backward pass is not implemented"):  # autograd: parameters that require grad
        net(x, t, condition=text)
    with pytest.raises(NotImplementedError, match="no autograd graph|backward pass"):
        net.few_step_sample(x, text, [0.9, 0.0])
    # CausalWan's own refusals stand as they were
    with pytest.raises(NotImplementedError, match="r_timestep=True"):
        CausalWan(r_timestep=True, **KW)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="skip_layers / r"):
        CausalWan(**KW)(x, t, condition=text, r=r)


# ---- 8. the per-block pin of the bidirectional call (tests/test_gpu_wan_full_blocks.py), what holds without a GPU --------------------
def _full_cases():
    import test_gpu_wan_full_blocks as FB

    return FB


@pytest.mark.parametrize("name", list(_full_cases().CASES))
def test_full_cases_reach_the_planned_kernels(name):
    """The matrix of tests/test_gpu_wan_full_blocks.py covers the kernel forms it names: the launcher's own plan (fg_op_attention_plan,
    scratch given as the engine gives it) for every case's self-attention (Lq == Lkv, ldk = D) and cross-attention (37 keys, ldk = 2 D)."""
    from fastgen_amd import _lib

    FB = _full_cases()
    c = FB.CASES[name]
    assert set(FB.PLANS) == set(FB.CASES)
    D, Ltok = 128 * c.heads, c.calls[0][2] * (c.lat[0] // 2) * (c.lat[1] // 2)
    got = []
    for Lkv, ldk in ((Ltok, D), (c.text_len, 2 * D)):
        p = _lib.fg_attention_plan()
        assert _lib.lib().fg_op_attention_plan(128, c.B, c.heads, Ltok, Lkv, ldk, 1, 0, 0, ctypes.byref(p)) == 0 and p.refusal == 0
        got.append((p.kernel, p.nsplit, p.t_cut, p.sample_major))
    assert tuple(got) == FB.PLANS[name], (name, got)
    # the last frame on the RoPE table's last row, unless the grid's rows / columns need a longer table
    assert all(k[0] == "full" and c.rope_max == max(k[2], c.lat[0] // 2, c.lat[1] // 2) for k in c.calls)


def test_full_matrix_names_every_kernel_form():
    from fastgen_amd._lib import FG_FA_TILE128, FG_FA_WIDE, FG_FA_WIDE_CUT

    FB = _full_cases()
    selfs = {v[0] for v in FB.PLANS.values()}
    assert {(FG_FA_TILE128, 1, 0, 0), (FG_FA_TILE128, 2, 0, 0), (FG_FA_TILE128, 1, 0, 1), (FG_FA_WIDE, 1, 0, 0), (FG_FA_WIDE, 3, 0, 0)} <= selfs
    cuts = {(n, FB.CASES[n].B) for n, v in FB.PLANS.items() if v[0][0] == FG_FA_WIDE_CUT}
    assert {b for _, b in cuts} == {2, 9}  # the cut at a batch > 1, and at B >= 8 past the sample-major limit ...
    assert FB.PLANS["F1056-B9"][1] == (FG_FA_TILE128, 1, 0, 0)  # ... where the cross-attention (Lq > 1024) leaves that map too


class OracleAsGpu:
    """`test_gpu_wan_blocks.Gpu`'s interface answered by the fp64 oracle itself - its own composition of the pieces, apart from
    run_case's: run_case then measures how far each mutant stands from the unmutated oracle (and that the two compositions agree:
    r term, skipped blocks, taps).  Calls of kind "full" only."""

    def __init__(self, c, cfg, sd):
        self.c, self.cfg = c, cfg
        self.p = {k[len("transformer."):]: v.double() for k, v in sd.items()}
        self.pr = {k.replace("r_embedder.", "condition_embedder."): v for k, v in self.p.items() if k.startswith("r_embedder.")}

    def set_text(self, text):
        self.ctx = R.text_embedding(self.p, text.double())

    def tapped(self, call, x, tf, rf=None):
        cfg, p = self.cfg, self.p
        kind, _, Fr, _, use_r, skip = call
        assert kind == "full"
        B, gh, gw = x.shape[0], x.shape[3] // 2, x.shape[4] // 2
        temb = R.time_embedding(p, cfg, tf.double().reshape(-1))
        tproj = R.time_projection(p, temb)
        if use_r:
            remb = R.time_embedding(self.pr, cfg, ((tf - rf) if self.c.r == "diff" else rf).double().reshape(-1))
            temb, tproj = temb + remb, tproj + R.time_projection(self.pr, remb)
        cos, sin = R.rope_for_chunk(cfg, Fr, gh, gw, 0, torch.float64)
        hs = R.patch_embed(p, x.double())
        r = dict(tokens=hs, temb=temb, tproj=tproj, blocks=[])
        for i in range(cfg.num_layers):
            if i in skip:
                r["blocks"].append(None)
                continue
            mod = R.modulation(p, i, tproj, B, Fr)
            q, k, v = R.self_attn_qkv(p, cfg, i, hs, mod, cos, sin)
            att1 = R.sdpa(q, k, v)
            x1 = R.self_attn_out(p, i, hs, att1, mod)
            att2, x2 = R.cross_attn(p, cfg, i, x1, *R.cross_kv(p, cfg, i, self.ctx))
            hs = R.ffn(p, cfg, i, x2, mod)
            r["blocks"].append(dict(attn1=att1, x_attn1=x1, attn2=att2, x_attn2=x2, x_ffn=hs))
        r["out"] = R.final_layer(p, cfg, hs, temb, Fr, gh, gw)
        return r

    def plain(self, call, x, tf, rf=None):
        return self.tapped(call, x, tf, rf)["out"]

    def close(self):
        pass


# the cases that carry a mutant of their own, and the small ones of the others ((m) - (q) are asserted on the GPU for every case)
@pytest.mark.parametrize("name", ["F105", "F555", "F105-C8", "R-diff", "R-abs", "SKIP"])
def test_full_block_mutants_stand_apart(name):
    """Every mutant of the per-block pin - the causal file's and (m) block-causal mask, (n) clamped RoPE, (o) per-sample r, (p) wrong r
    term, (q) skip ignored - differs from the unmutated fp64 oracle by at least MUTANT_FACTOR x the bound of the quantity it is checked
    on, in the granule used, at the seeds the GPU test runs: the inputs are adequate.  (`rep.bad` also holds any disagreement of
    run_case's composition with OracleAsGpu's.)"""
    FB = _full_cases()
    rep = FB.run_case(FB.CASES[name], OracleAsGpu, FB.TOL_FULL)
    FB.report(name, rep)
    assert not rep.bad, rep.bad
    want = {"F105": {"m:attn1", "n:attn1"}, "F555": {"m:attn1", "n:attn1"}, "F105-C8": {"m:attn1", "n:attn1", "a:inc1", "f:attn2"},
            "SKIP": {"q:inc1", "q:out", "m:attn1"},
            "R-diff": {f"{m}:{q}" for m in ("o", "p:ignore_r", "p:swap_cond") for q in ("temb", "tproj")}
            | {f"p:{m}:{q}" for m in ("ignore_r", "swap_cond") for q in ("inc1", "ffn")} | {"p:proj_only:temb", "p:proj_only:out"}}
    want["R-abs"] = want["R-diff"]
    assert want[name] | {"b:inc1", "b:ffn", "d:attn1", "e:attn1"} <= set(rep.mut), sorted(rep.mut)
    assert all(v >= FB.MUTANT_FACTOR for v in rep.mut.values()), rep.mut
