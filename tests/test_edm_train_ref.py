"""CPU checks of tests/edm_train_ref.py, the fp64 references the GPU tests of the EDM training kernels compare against
(test_gpu_edm_train_ops.py): (1) the written-out formulas equal torch.autograd / torch.func in fp64, so the reference itself is pinned;
(2) on every input the bound is small against the values - median(bound / max|value|) <= 2^-12 in fp32 storage, 2^-6 in bf16 - so it
cannot hide a failure; (3) each input family rejects the named mutations of the reference: a mutated reference differs from the true
one by more than the bound on at least one element of the element class named here; (4) the entry points refuse, before any launch,
the shapes their launchers cannot serve."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from fastgen_amd import _lib

import edm_train_ref as R

F64 = torch.float64
LIMIT = {0: 2.0 ** -12, 1: 2.0 ** -6}
DT_NAME = {0: "fp32", 1: "bf16"}


def case_id(c):
    return "-".join(str(int(v) if isinstance(v, bool) else v) for v in c)


def cpu_keep(shape, p):
    """A stand-in for the device's dropout mask (the GPU tests take the real one from fg_op_dropout_mask)."""
    if p <= 0:
        return None
    return (torch.rand(shape, generator=torch.Generator().manual_seed(5), dtype=F64) >= p).to(F64) / (1.0 - p)


def gn_refs(case, dtype, mut=None):
    c1, c2, res, B, mode, rm, add, acc, _, p, _ = case
    C, ro = c1 + c2, R.gn_out_res(res, rm)
    d = R.gn_inputs(case, dtype)
    out = dict(R.gn_backward(d["x"], d["dact"], d["gamma"], d["beta"], R.GN_EPS, mode, rm, cpu_keep((B, res, res, C), p), d["add"], 0.7,
                             d["old"], dtype, d["dg_old"], d["db_old"], mut=mut))
    out["act"] = R.gn_act(d["x"], d["gamma"], d["beta"], R.GN_EPS, mode, rm, cpu_keep((B, ro, ro, C), p), dtype, mut=mut)
    out["jvp"] = R.gn_jvp(d["x"], d["xd"], d["gamma"], d["beta"], R.GN_EPS, mode, cpu_keep((B, res, res, C), p), dtype, mut=mut)
    return out


def attn_refs(case, dtype, mut=None):
    d = R.attn_inputs(case, dtype)
    out = dict(R.attention_backward(d["q"], d["k"], d["vt"], d["dO"], dtype, mut=mut))
    out["od"] = R.attention_jvp(d["q"], d["k"], d["vt"], d["qd"], d["kd"], d["vtd"], dtype, mut=mut)
    return out


# ---- (1) the references against autograd ----------------------------------------------------------------------------------------------

def close(a, b, tol=1e-10):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


def _gn_forward(x, gamma, beta, mode, rm, keep, C):
    """x NHWC fp64 -> the conv operand, NHWC at the output resolution, by torch's own group_norm / silu / pooling."""
    G, _ = R.gn_geometry(C)
    y = F.group_norm(x.permute(0, 3, 1, 2).contiguous(), G, gamma, beta, R.GN_EPS)
    if mode == 0:
        y = F.silu(y)
    if rm == 1:
        y = F.avg_pool2d(y, 2)
    elif rm == 2:
        y = F.interpolate(y, scale_factor=2, mode="nearest")
    y = y.permute(0, 2, 3, 1)
    return y if keep is None else y * keep


@pytest.mark.parametrize("case", [R.GN_CASES[i] for i in (1, 2, 3, 7, 8, 9)], ids=case_id)
def test_gn_references_equal_autograd(case):
    c1, c2, res, B, mode, rm, add, acc, _, p, params = case
    C, ro = c1 + c2, R.gn_out_res(res, rm)
    d = R.gn_inputs(case, 0)
    x, gamma, beta = d["x"].clone().requires_grad_(), d["gamma"].clone().requires_grad_(), d["beta"].clone().requires_grad_()
    keep_out, keep_in = cpu_keep((B, ro, ro, C), p), cpu_keep((B, res, res, C), p)
    close(R.gn_act(d["x"], d["gamma"], d["beta"], R.GN_EPS, mode, rm, keep_out, 0)[0], _gn_forward(x, gamma, beta, mode, rm, keep_out, C).detach())
    # backward: the dropout sits between the activation and the resampling (UNetBlock.forward), i.e. at the norm's resolution
    G, _ = R.gn_geometry(C)
    y = F.group_norm(x.permute(0, 3, 1, 2).contiguous(), G, gamma, beta, R.GN_EPS)
    a = (F.silu(y) if mode == 0 else y).permute(0, 2, 3, 1)
    if keep_in is not None:
        a = a * keep_in
    resample = lambda t: t if rm == 0 else (F.avg_pool2d(t.permute(0, 3, 1, 2), 2) if rm == 1 else F.interpolate(t.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")).permute(0, 2, 3, 1)
    loss = (resample(a) * d["dact"]).sum()
    if add:
        loss = loss + 0.7 * (resample(x) * d["add"]).sum()
    gx, gg, gb = torch.autograd.grad(loss, (x, gamma, beta))
    ref = R.gn_backward(d["x"], d["dact"], d["gamma"], d["beta"], R.GN_EPS, mode, rm, keep_in, d["add"], 0.7, d["old"], 0, d["dg_old"], d["db_old"])
    close(ref["dx"][0], gx + (d["old"] if acc else 0.0), 1e-9)
    if params:
        close(ref["dgamma"][0], gg + d["dg_old"], 1e-9)
        close(ref["dbeta"][0], gb + d["db_old"], 1e-9)
    f = lambda t: (lambda v: v if keep_in is None else v * keep_in)((F.silu if mode == 0 else (lambda u: u))(
        F.group_norm(t.permute(0, 3, 1, 2).contiguous(), G, d["gamma"], d["beta"], R.GN_EPS)).permute(0, 2, 3, 1))
    _, tangent = torch.func.jvp(f, (d["x"],), (d["xd"],))
    close(R.gn_jvp(d["x"], d["xd"], d["gamma"], d["beta"], R.GN_EPS, mode, keep_in, 0)[0], tangent, 1e-9)


@pytest.mark.parametrize("case", [R.ATTN_CASES[i] for i in (0, 1, 2, 4)], ids=case_id)
def test_attention_references_equal_autograd(case):
    T, C, B, _ = case
    d = R.attn_inputs(case, 0)
    sc = float(torch.tensor(1.0 / math.sqrt(C), dtype=torch.float32))  # the kernels' fp32 scale
    fwd = lambda q, k, vt: torch.softmax(sc * (q @ k.transpose(1, 2)), -1) @ vt.transpose(1, 2)
    q, k, vt = (d[n].clone().requires_grad_() for n in ("q", "k", "vt"))
    gq, gk, gvt = torch.autograd.grad((fwd(q, k, vt) * d["dO"]).sum(), (q, k, vt))
    ref = R.attention_backward(d["q"], d["k"], d["vt"], d["dO"], 0)
    for name, g in (("dq", gq), ("dk", gk), ("dvt", gvt)):
        close(ref[name][0], g, 1e-9)
    _, tangent = torch.func.jvp(fwd, (d["q"], d["k"], d["vt"]), (d["qd"], d["kd"], d["vtd"]))
    close(R.attention_jvp(d["q"], d["k"], d["vt"], d["qd"], d["kd"], d["vtd"], 0)[0], tangent, 1e-9)


def test_linear_reference_equals_autograd():
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    dy, x, w, b = rn(5, 100), rn(5, 512).requires_grad_(), rn(100, 512).requires_grad_(), rn(100).requires_grad_()
    gx, gw, gb = torch.autograd.grad((F.linear(x, w, b) * dy).sum(), (x, w, b))
    dw0, db0, dx0 = rn(100, 512), rn(100), rn(5, 512)
    ref = R.linear_backward(dy, x.detach(), w.detach(), dw0, db0, dx0, 0.625)
    close(ref["dw"][0], dw0 + 0.625 * gw)
    close(ref["db"][0], db0 + gb)
    close(ref["dx"][0], dx0 + gx)


def test_silu_and_coef_references_equal_autograd():
    pre = torch.linspace(-20, 20, 401, dtype=F64).requires_grad_()
    (g,) = torch.autograd.grad(F.silu(pre).sum(), pre)
    close(R.silu_bwd(torch.ones(401, dtype=F64), pre.detach())[0], g)
    # the preconditioning coefficients' t-derivatives (EDMPrecond: c_in, c_noise = ln(t) / 4, c_skip, c_out with the shifted t)
    t = torch.tensor([0.002, 80.0, 0.5, 1.0], dtype=F64)
    sd, sh = 0.5, 0.25
    fs = [lambda t: (sd * sd + t * t) ** -0.5, lambda t: torch.log(t) / 4, lambda t: sd * sd / ((t - sh) ** 2 + sd * sd),
          lambda t: (t - sh) * sd / ((t - sh) ** 2 + sd * sd).sqrt()]
    vt = torch.tensor([1.0, -2.0, 0.5, 3.0], dtype=F64)
    v, _ = R.jvp_coef(t, None, vt, None, sd, sh, 0)
    for row, val_row, f in ((1, 0, fs[0]), (2, None, fs[1]), (5, 4, fs[2]), (7, 6, fs[3])):
        val, tan = torch.func.jvp(f, (t,), (vt,))
        close(v[row], tan)
        if val_row is not None:
            close(v[val_row], val)


# ---- (2) the bounds are small against the values -------------------------------------------------------------------------------------------

def assert_bound_small(tag, v, b, dtype):
    assert torch.isfinite(b).all() and (b >= 0).all(), tag
    top = v.abs().max().item()
    if top == 0.0:  # an identically zero result (dk at q = 0) is computed exactly
        assert b.max().item() == 0.0, tag
        return
    assert (b / top).median().item() <= LIMIT[dtype], (tag, (b / top).median().item() / LIMIT[dtype])


@pytest.mark.parametrize("dtype", [0, 1], ids=DT_NAME.get)
def test_bounds_are_small_against_the_values(dtype):
    for case in R.GN_CASES + R.GN_SWEEP:
        for name, (v, b) in gn_refs(case, dtype).items():
            assert_bound_small(f"gn {case_id(case)} {name}", v, b, dtype)
    for case in R.ATTN_CASES:
        for name, (v, b) in attn_refs(case, dtype).items():
            assert_bound_small(f"attention {case_id(case)} {name}", v, b, dtype)
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    for C, HW, B in [(C, HW, B) for C in (8, 72, 256) for HW in (16, 64, 1024) for B in (1, 4, 5, 9)]:
        assert_bound_small("colsum", *R.colsum(R.as_storage(rn(B, HW, C), dtype), 0.375), 0)
        assert_bound_small("batchsum_add", *R.batchsum_add(rn(B, C), rn(C)), 0)
    for B, C, K in [(1, 8, 16), (5, 100, 512), (3, 256, 512)]:
        for name, (v, b) in R.linear_backward(rn(B, C), rn(B, K), rn(C, K), rn(C, K), rn(C), rn(B, K), 0.625).items():
            assert_bound_small(f"linear {name}", v, b, 0)


# ---- (3) the inputs reject the mutations ----------------------------------------------------------------------------------------------------

def exceeds(true, mutated):
    """Elements where the mutated reference leaves the true one's bound."""
    (v, b), (m, _) = true, mutated
    return (m - v).abs() > b


def straddle_upper(C):
    """Channels whose group differs from the group of their octet's first channel."""
    _, cpg = R.gn_geometry(C)
    c = torch.arange(C)
    return (c // cpg) != ((c // 8) * 8) // cpg


# mutation -> (which GN cases it must be caught on, outputs that must catch it, the element class that catches it)
GN_CATCH = {
    "no_s2": (lambda c: True, ("dx", "jvp"), "any element: the xhat S2 term reaches every pixel"),
    "octet_g0": (lambda c: c[0] + c[1] in (16, 96, 384), ("dx", "jvp"), "the channels of an octet's upper group (cpg 4 and 12)"),
    "rm1_no_quarter": (lambda c: c[5] == 1, ("dx",), "any element of a down-sampling case"),
    "rm2_three": (lambda c: c[5] == 2, ("dx",), "any element of an up-sampling case"),
    "batch_ge4_dropped": (lambda c: c[3] >= 5 and c[10], ("dgamma", "dbeta"), "the per-channel sums at batch 5"),
    "stats_image0": (lambda c: c[3] > 1, ("dx", "jvp"), "the images n >= 1 (the last one is 1000 x larger)"),
    "mask_shift_octet": (lambda c: c[9] > 0, ("dx", "jvp", "act"), "elements whose keep factor differs from the one eight elements before"),
}


def test_every_named_mutation_has_its_inputs():
    assert set(GN_CATCH) == set(R.GN_MUTATIONS) and set(ATTN_CATCH) == set(R.ATTN_MUTATIONS)


@pytest.mark.parametrize("dtype", [0, 1], ids=DT_NAME.get)
@pytest.mark.parametrize("mut", sorted(GN_CATCH))
def test_gn_inputs_reject_mutation(mut, dtype):
    applies, outputs, _ = GN_CATCH[mut]
    cases = [c for c in R.GN_CASES if applies(c)]
    assert cases
    for case in cases:
        true, bad = gn_refs(case, dtype), gn_refs(case, dtype, mut)
        C, B = case[0] + case[1], case[3]
        for name in outputs:
            if name not in true:
                continue
            hit = exceeds(true[name], bad[name])
            assert hit.any(), (mut, case_id(case), name)
            if mut == "octet_g0":  # nothing but the upper channels of straddling octets moves
                assert not hit[..., ~straddle_upper(C)].any() and hit[..., straddle_upper(C)].any()
            if mut == "stats_image0":
                assert not hit[0].any() and all(hit[n].any() for n in range(1, B))
        if mut == "batch_ge4_dropped":  # dx does not depend on the batch sums
            assert not exceeds(true["dx"], bad["dx"]).any()


def test_unclamped_g1_reads_no_statistic_a_channel_uses():
    """load_oct_coef clamps g1 = g0 + 1 at the last group.  The clamp only keeps the LOAD inside mr / S: a channel selects g1 when
    rem + j >= cpg, and then its own group is g0 + 1 <= groups - 1, so no result depends on the clamped value and no input can reject
    that mutation through an output.  This checks the argument for every width the tests and the network use."""
    for C in (16, 96, 128, 256, 384, 512, 768):
        G, cpg = R.gn_geometry(C)
        assert cpg == 4 or cpg >= 8
        for c0 in range(0, C, 8):
            g0, rem = c0 // cpg, c0 % cpg
            for j in range(8):
                sel = g0 + (1 if rem + j >= cpg else 0)
                assert sel == (c0 + j) // cpg and sel <= G - 1


ATTN_CATCH = {
    "dk_from_ds": (lambda c: True, ("dk",), "dk rows (dS is not symmetric)"),
    "softmax_first_wave": (lambda c: c[0] == 256, ("dq", "dk", "dvt", "od"), "every row at T = 256 (the sum misses three of four waves)"),
    "dv_untransposed": (lambda c: True, ("dvt",), "dvt off the diagonal"),
    "jvp_no_pvd": (lambda c: True, ("od",), "every element of od"),
}


@pytest.mark.parametrize("dtype", [0, 1], ids=DT_NAME.get)
@pytest.mark.parametrize("mut", sorted(ATTN_CATCH))
def test_attention_inputs_reject_mutation(mut, dtype):
    applies, outputs, _ = ATTN_CATCH[mut]
    for case in R.ATTN_CASES:
        true, bad = attn_refs(case, dtype), attn_refs(case, dtype, mut)
        for name in outputs:
            hit = exceeds(true[name], bad[name])
            if applies(case) and not (name == "dk" and case[3] == "q0"):  # q = 0: dk is zero either way
                assert hit.any(), (mut, case_id(case), name)
            elif mut == "softmax_first_wave":  # T = 64: one wave is the whole row
                assert not hit.any()


def test_sums_and_weights_reject_mutations():
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    for B in (5, 9):
        inp, old = rn(B, 72), rn(72)
        assert exceeds(R.batchsum_add(inp, old), R.batchsum_add(inp, old, mut="batch_ge4_dropped")).all()
    inp, old = rn(4, 72), rn(72)
    assert not exceeds(R.batchsum_add(inp, old), R.batchsum_add(inp, old, mut="batch_ge4_dropped")).any()
    w = rn(24, 8, 9)
    good, bad = R.dgrad_weights(w, 256), R.dgrad_weights(w, 256, mut="no_tap_flip")
    assert (good != bad)[:8, :, [0, 1, 2, 3, 5, 6, 7, 8]].all() and torch.equal(good[:, :, 4], bad[:, :, 4])  # every tap but the centre
    w1 = rn(128, 256, 1)
    assert torch.equal(R.dgrad_weights(w1, 256), R.dgrad_weights(w1, 256, mut="no_tap_flip"))


# ---- (4) refusals before any launch ----------------------------------------------------------------------------------------------------------

def test_entry_points_refuse_what_the_launchers_cannot_serve():
    L = _lib.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    base = buf.data_ptr()
    one = ctypes.c_void_p(base + (-base) % 256)
    big = 1 << 40  # claimed sizes: nothing is launched, nothing is touched
    assert L.fg_op_gn_workspace_bytes(3, 192) == 0 and L.fg_op_gn_workspace_bytes(3, 8) == 0 and L.fg_op_gn_workspace_bytes(3, 96) > 0
    for C in (192, 8):  # cpg 6; fewer than 16 channels
        with pytest.raises(_lib.FastGenAMDError, match="group size"):
            _lib.check(L.fg_op_gn_backward(0, 0, one, C, None, 0, one, C, one, one, 1e-6, None, None, None, 0, 0.0, one, None, 0, 3, 8, 0, 0.0, 0, 0,
                                           one, big, None))
        with pytest.raises(_lib.FastGenAMDError, match="group size"):
            _lib.check(L.fg_op_gn_jvp(0, 0, one, C, None, 0, one, one, one, 1e-6, one, 3, 8, 0.0, 0, 0, one, big, None))
        with pytest.raises(_lib.FastGenAMDError, match="GroupNorm"):
            _lib.check(L.fg_op_gn_act(0, 0, one, C, None, 0, one, one, 1e-6, one, 3, 8, 0, 0.0, 0, 0, one, big, None))
    with pytest.raises(_lib.FastGenAMDError, match="workspace too small"):
        _lib.check(L.fg_op_gn_backward(0, 0, one, 96, None, 0, one, 96, one, one, 1e-6, None, None, None, 0, 0.0, one, None, 0, 3, 8, 0, 0.0, 0, 0,
                                       one, 64, None))
    with pytest.raises(_lib.FastGenAMDError, match="pitches"):
        _lib.check(L.fg_op_gn_backward(0, 0, one, 96, None, 0, one, 88, one, one, 1e-6, None, None, None, 0, 0.0, one, None, 0, 3, 8, 0, 0.0, 0, 0,
                                       one, big, None))
    with pytest.raises(_lib.FastGenAMDError, match="even with rm 1"):
        _lib.check(L.fg_op_gn_backward(0, 0, one, 96, None, 0, one, 96, one, one, 1e-6, None, None, None, 0, 0.0, one, None, 0, 3, 7, 1, 0.0, 0, 0,
                                       one, big, None))
    for T, C in ((128, 32), (32, 32), (64, 40)):
        assert L.fg_op_attention_backward_workspace_bytes(1, 3, T, C) == 0
        with pytest.raises(_lib.FastGenAMDError, match="unsupported"):
            _lib.check(L.fg_op_attention_backward(1, one, one, one, one, one, one, one, None, 3, T, C, one, big, None))
        with pytest.raises(_lib.FastGenAMDError, match="unsupported"):
            _lib.check(L.fg_op_attention_jvp(1, one, one, one, one, one, one, one, 3, T, C, one, big, None))
    assert L.fg_op_attention_backward_workspace_bytes(1, 3, 64, 256) > 0
    with pytest.raises(_lib.FastGenAMDError, match="workspace too small"):
        _lib.check(L.fg_op_attention_jvp(1, one, one, one, one, one, one, one, 3, 64, 256, one, 1024, None))
    with pytest.raises(_lib.FastGenAMDError, match="fg_op_colsum"):
        _lib.check(L.fg_op_colsum(0, one, 64, 72, one, 2, 16, 1.0, 0, None))  # ct < c
    with pytest.raises(_lib.FastGenAMDError, match="fg_op_colsum"):
        _lib.check(L.fg_op_colsum(0, one, 16, 12, one, 2, 16, 1.0, 0, None))  # c % 8
    with pytest.raises(_lib.FastGenAMDError, match="in_stride"):
        _lib.check(L.fg_op_batchsum_add(one, one, None, 4, 72, 64, None))
    for db, dx in ((one, None), (None, one)):  # only the weight gradient takes a row stride
        with pytest.raises(_lib.FastGenAMDError, match="row stride"):
            _lib.check(L.fg_op_linear_backward(0, one, one, one, None, db, dx, 3, 100, 512, 1.0, 107, None))
    with pytest.raises(_lib.FastGenAMDError, match="embedding-affine"):
        _lib.check(L.fg_op_linear_backward(1, one, one, one, one, one, None, 3, 100, 512, 1.0, 0, None))
    with pytest.raises(_lib.FastGenAMDError, match="cin_pad"):
        _lib.check(L.fg_op_dgrad_weights(one, one, 128, 64, 32, 9, None))
    with pytest.raises(_lib.FastGenAMDError, match="unknown op"):
        _lib.check(L.fg_op_train_elementwise(99, 0, one, one, one, one, one, one, 1, 3, 8, 64, 0.0, 0.0, 0, None))
    with pytest.raises(_lib.FastGenAMDError, match="ch_pad"):
        _lib.check(L.fg_op_train_elementwise(_lib.FG_TRAIN_OP_HEAD_GRAD, 0, one, one, None, None, None, one, 1, 8, 3, 64, 0.0, 0.0, 0, None))
