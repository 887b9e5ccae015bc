"""Per-op, per-element parity of the EDM training kernels (fastgen_amd/csrc/bwd.hip, attn_bwd.hip) through the fg_op_* entry points
over their launchers, each against the plain fp64 reference of tests/edm_train_ref.py: |got - ref| <= bound for EVERY element, in
both storage types (fp32 = the bf16x3 mode's, bf16).  Outputs are pre-filled with NaN (the accumulate forms with prior values) and
the padding of pitched operands is NaN, so an element that is not written, or a read past a tensor's channels, fails.  The composite
tests (test_gpu_parity.py) judge these kernels by relative L2 over whole tensors at batch 1 or 2 and T = 256 only; the shapes here are
the batch tails, T = 64, the group / octet geometries and the resampling modes those cannot see (edm_train_ref.GN_CASES, GN_SWEEP,
ATTN_CASES).  test_edm_train_ref.py shows on the CPU that these inputs reject the named mutations of the reference.

Each check prints `HEADROOM <op> <storage> <case> <output> <worst |err| / bound>` (DESIGN.md's table)."""
import math

import pytest
import torch

from fastgen_amd import _lib

import edm_train_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
DTYPES = [0, 1]
DT_NAME = {0: "fp32", 1: "bf16"}
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def tdt(dtype):
    return torch.bfloat16 if dtype else torch.float32


def act(t, dtype):
    """fp64 values (exact in the storage type) -> a device tensor of the storage type."""
    return t.to(tdt(dtype)).contiguous().to(dev())


def f32(t):
    return None if t is None else t.to(torch.float32).contiguous().to(dev())


def pitched(t, pitch, dtype):
    """[.., C] -> device [.., pitch] of the storage type with NaN in the padding channels."""
    out = torch.full(t.shape[:-1] + (pitch,), NAN, dtype=tdt(dtype))
    out[..., : t.shape[-1]] = t.to(tdt(dtype))
    return out.to(dev())


def ptr(t):
    return None if t is None else t.data_ptr()


def back(t):
    torch.cuda.synchronize()
    return t.detach().cpu().to(F64)


def check(tag, got, ref, bound):
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{tag}: {(~torch.isfinite(got)).sum().item()} elements not written (NaN)"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = ratio.max().item()
    print(f"HEADROOM {tag} {worst:.4f}")
    if worst > 1.0:
        i = ratio.argmax().item()
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError(f"{tag}: {(ratio > 1).sum().item()} of {ratio.numel()} elements outside the bound; worst at {idx}: got "
                             f"{got.flatten()[i].item():.9g}, ref {ref.flatten()[i].item():.9g}, bound {bound.flatten()[i].item():.3g}")


def gn_ws(B, C):
    n = _lib.lib().fg_op_gn_workspace_bytes(B, C)
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=dev()), n


def keep_factors(shape, p):
    """The dropout keep factors of the operand `shape` ([B, H, W, C], flattened), from fg_op_dropout_mask (pinned in test_gpu_parity.py)."""
    if p <= 0:
        return None
    m = torch.empty(shape, dtype=torch.float32, device=dev())
    _lib.check(_lib.lib().fg_op_dropout_mask(m.data_ptr(), m.numel(), p, R.DROP_BLOCK, R.DROP_SEED, None))
    return back(m)


def case_id(c):
    return "-".join(str(int(v) if isinstance(v, bool) else v) for v in c)


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("case", R.GN_CASES + R.GN_SWEEP, ids=case_id)
def test_gn_backward(case, dtype):
    """fg_op_gn_backward -> launch_gn_coeffs + launch_gn_bwd: gn_bwd_reduce_kernel, gn_bwd_group(_param)_kernel, gn_bwd_apply_kernel."""
    c1, c2, res, B, mode, rm, add, acc, use_dx2, p, params = case
    C, ro = c1 + c2, R.gn_out_res(res, rm)
    d = R.gn_inputs(case, dtype)
    L = _lib.lib()
    x1 = act(d["x"][..., :c1], dtype)
    x2 = act(d["x"][..., c1:], dtype) if c2 else None
    cd, ca = C + 8, C + 24
    dact = pitched(d["dact"], cd, dtype)
    addt = pitched(d["add"], ca, dtype) if add else None
    first = d["old"] if acc else torch.full((B, res, res, C), NAN, dtype=F64)
    if use_dx2:
        dx, dx2 = act(first[..., :c1], dtype), act(first[..., c1:], dtype)
    else:
        dx, dx2 = act(first, dtype), None
    dg, db = f32(d["dg_old"]), f32(d["db_old"])
    gamma, beta = f32(d["gamma"]), f32(d["beta"])
    ws, nws = gn_ws(B, C)
    keep = keep_factors((B, res, res, C), p)
    _lib.check(L.fg_op_gn_backward(dtype, mode, x1.data_ptr(), c1, ptr(x2), c2, dact.data_ptr(), cd, gamma.data_ptr(), beta.data_ptr(), R.GN_EPS,
                                   ptr(dg), ptr(db), ptr(addt), ca, 0.7, dx.data_ptr(), ptr(dx2), int(acc), B, res, rm, p, R.DROP_BLOCK,
                                   R.DROP_SEED, ws.data_ptr(), nws, None))
    got = {"dx": torch.cat([back(dx), back(dx2)], -1) if use_dx2 else back(dx)}
    if params:
        got["dgamma"], got["dbeta"] = back(dg), back(db)
    ref = R.gn_backward(d["x"], d["dact"], d["gamma"], d["beta"], R.GN_EPS, mode, rm, keep, d["add"], float(torch.tensor(0.7, dtype=torch.float32)),
                        d["old"] if acc else None, dtype, d["dg_old"], d["db_old"])
    assert set(ref) == set(got)
    for name in got:
        check(f"gn_backward {DT_NAME[dtype]} {case_id(case)} {name}", got[name], *ref[name])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("case", R.GN_CASES + R.GN_SWEEP, ids=case_id)
def test_gn_act(case, dtype):
    """fg_op_gn_act -> launch_gn_act: gn_act_kernel<0 | 1> of the case, and gn_act_kernel<2> (the plain resampled copy) on the same x."""
    c1, c2, res, B, mode, rm, _, _, _, p, _ = case
    C, ro = c1 + c2, R.gn_out_res(res, rm)
    d = R.gn_inputs(case, dtype)
    L = _lib.lib()
    x1 = act(d["x"][..., :c1], dtype)
    x2 = act(d["x"][..., c1:], dtype) if c2 else None
    gamma, beta = f32(d["gamma"]), f32(d["beta"])
    ws, nws = gn_ws(B, C)
    keep = keep_factors((B, ro, ro, C), p)
    for m, pm, km in ((mode, p, keep), (2, 0.0, None)):
        out = torch.full((B, ro, ro, C), NAN, dtype=tdt(dtype), device=dev())
        _lib.check(L.fg_op_gn_act(dtype, m, x1.data_ptr(), c1, ptr(x2), c2, gamma.data_ptr(), beta.data_ptr(), R.GN_EPS, out.data_ptr(), B, ro, rm,
                                  pm, R.DROP_BLOCK, R.DROP_SEED, ws.data_ptr(), nws, None))
        check(f"gn_act {DT_NAME[dtype]} {case_id(case)} mode{m}", back(out), *R.gn_act(d["x"], d["gamma"], d["beta"], R.GN_EPS, m, rm, km, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("case", R.GN_CASES + R.GN_SWEEP, ids=case_id)
def test_gn_jvp(case, dtype):
    """fg_op_gn_jvp -> launch_gn_jvp: gn_bwd_reduce_kernel<1>, gn_bwd_group_kernel (unweighted), gn_jvp_apply_kernel."""
    c1, c2, res, B, mode, _, _, _, _, p, _ = case
    C = c1 + c2
    d = R.gn_inputs(case, dtype)
    L = _lib.lib()
    x1 = act(d["x"][..., :c1], dtype)
    x2 = act(d["x"][..., c1:], dtype) if c2 else None
    xd = act(d["xd"], dtype)
    gamma, beta = f32(d["gamma"]), f32(d["beta"])
    ws, nws = gn_ws(B, C)
    keep = keep_factors((B, res, res, C), p)
    out = torch.full((B, res, res, C), NAN, dtype=tdt(dtype), device=dev())
    _lib.check(L.fg_op_gn_jvp(dtype, mode, x1.data_ptr(), c1, ptr(x2), c2, xd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), R.GN_EPS, out.data_ptr(),
                              B, res, p, R.DROP_BLOCK, R.DROP_SEED, ws.data_ptr(), nws, None))
    check(f"gn_jvp {DT_NAME[dtype]} {case_id(case)} out", back(out), *R.gn_jvp(d["x"], d["xd"], d["gamma"], d["beta"], R.GN_EPS, mode, keep, dtype))


# ---- attention ------------------------------------------------------------------------------------------------------------------

def attn_ws(dtype, B, T, C):
    n = _lib.lib().fg_op_attention_backward_workspace_bytes(dtype, B, T, C)
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=dev()), n


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=case_id)
def test_attention_backward(case, dtype):
    """fg_op_attention_backward -> launch_attention_backward (transposes, nt_gemm_kernel, softmax_rows_kernel, attn_ds_kernel) and
    launch_qkv_interleave; dq, dk, dvt one by one, the interleave bit-identical to the three planes."""
    T, C, B, _ = case
    d = R.attn_inputs(case, dtype)
    L = _lib.lib()
    q, k, vt, dO = (act(d[n], dtype) for n in ("q", "k", "vt", "dO"))
    new = lambda *s: torch.full(s, NAN, dtype=tdt(dtype), device=dev())
    dq, dk, dvt, dqkv = new(B, T, C), new(B, T, C), new(B, C, T), new(B, T, 3 * C)
    ws, nws = attn_ws(dtype, B, T, C)
    _lib.check(L.fg_op_attention_backward(dtype, q.data_ptr(), k.data_ptr(), vt.data_ptr(), dO.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                          dvt.data_ptr(), dqkv.data_ptr(), B, T, C, ws.data_ptr(), nws, None))
    ref = R.attention_backward(d["q"], d["k"], d["vt"], d["dO"], dtype)
    got = {"dq": back(dq), "dk": back(dk), "dvt": back(dvt)}
    for name in ("dq", "dk", "dvt"):
        check(f"attention_backward {DT_NAME[dtype]} {case_id(case)} {name}", got[name], *ref[name])
    planes = torch.stack([got["dq"], got["dk"], got["dvt"].transpose(1, 2)], -1).reshape(B, T, 3 * C)  # channel c * 3 + plane
    assert torch.equal(back(dqkv), planes)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=case_id)
def test_attention_jvp(case, dtype):
    """fg_op_attention_jvp -> launch_attention_jvp; T 64 with C 256 takes its C > T branch (the two fp32 products in the transposes' space)."""
    T, C, B, _ = case
    d = R.attn_inputs(case, dtype)
    L = _lib.lib()
    q, k, vt, qd, kd, vtd = (act(d[n], dtype) for n in ("q", "k", "vt", "qd", "kd", "vtd"))
    od = torch.full((B, T, C), NAN, dtype=tdt(dtype), device=dev())
    ws, nws = attn_ws(dtype, B, T, C)
    _lib.check(L.fg_op_attention_jvp(dtype, q.data_ptr(), k.data_ptr(), vt.data_ptr(), qd.data_ptr(), kd.data_ptr(), vtd.data_ptr(), od.data_ptr(),
                                     B, T, C, ws.data_ptr(), nws, None))
    check(f"attention_jvp {DT_NAME[dtype]} {case_id(case)} od", back(od),
          *R.attention_jvp(d["q"], d["k"], d["vt"], d["qd"], d["kd"], d["vtd"], dtype))


# ---- column and batch sums ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("B", [1, 4, 5, 9])
@pytest.mark.parametrize("HW", [16, 64, 1024])
@pytest.mark.parametrize("C", [8, 72, 256])
def test_colsum(C, HW, B, dtype):
    """fg_op_colsum -> launch_colsum: ct > C with NaN padding, a row stride on the output, a scale; C 72: the second workgroup has one octet."""
    g = torch.Generator().manual_seed(C + HW + B)
    t = R.as_storage(torch.randn(B, HW, C, generator=g, dtype=F64), dtype)
    ct, stride, scale = C + 16, C + 5, 0.375
    out = torch.full((B, stride), NAN, dtype=torch.float32, device=dev())
    tp = pitched(t, ct, dtype)
    _lib.check(_lib.lib().fg_op_colsum(dtype, tp.data_ptr(), ct, C, out.data_ptr(), B, HW, scale, stride, None))
    got = back(out)
    assert torch.isnan(got[:, C:]).all()  # nothing written between the rows
    check(f"colsum {DT_NAME[dtype]} {C}-{HW}-{B} out", got[:, :C], *R.colsum(t, scale))


@pytest.mark.parametrize("B", [1, 4, 5, 9])
@pytest.mark.parametrize("C", [8, 72, 100, 256])
def test_batchsum_add(C, B):
    """fg_op_batchsum_add -> launch_batchsum_add: a row stride on the input (NaN between the rows), two destinations with different priors."""
    g = torch.Generator().manual_seed(C + B)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64).float().to(F64)
    inp, o1, o2 = rn(B, C), rn(C), 3.0 * rn(C)
    stride = C + 3
    d_in = torch.full((B, stride), NAN, dtype=torch.float32)
    d_in[:, :C] = inp.float()
    d_in, d1, d2 = d_in.to(dev()), f32(o1), f32(o2)
    _lib.check(_lib.lib().fg_op_batchsum_add(d_in.data_ptr(), d1.data_ptr(), d2.data_ptr(), B, C, stride, None))
    check(f"batchsum_add fp32 {C}-{B} out", back(d1), *R.batchsum_add(inp, o1))
    check(f"batchsum_add fp32 {C}-{B} out2", back(d2), *R.batchsum_add(inp, o2))
    d3 = f32(o1)
    _lib.check(_lib.lib().fg_op_batchsum_add(d_in.data_ptr(), d3.data_ptr(), None, B, C, stride, None))
    assert torch.equal(back(d3), back(d1))


# ---- linear / affine backward, data-gradient weights --------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["dw", "db", "dx", "all", "affine_dw", "affine_dx", "affine_all", "dw_stride"])
@pytest.mark.parametrize("B,C,K", [(1, 8, 16), (5, 100, 512), (3, 256, 512), (9, 100, 16)])
def test_linear_backward(B, C, K, which):
    """fg_op_linear_backward -> launch_linear_bwd (linear_wgrad_kernel, batchsum_add_kernel, affine_dgrad_kernel) and launch_affine_bwd
    (affine_wgrad_kernel, affine_dgrad_kernel), each output alone and together, accumulating into non-zero values.  B 9: the 8-row
    body and the tail of linear_wgrad_kernel; C 100: the 8-row body and the tail of affine_dgrad_kernel."""
    g = torch.Generator().manual_seed(B + C + K)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64).float().to(F64)
    dy, x, w = rn(B, C), rn(B, K), rn(C, K)
    affine = which.startswith("affine")
    want = which.split("_")[-1]
    dw0 = rn(C, K) if want in ("dw", "all", "stride") else None
    db0 = rn(C) if want in ("db", "all") and not affine else None
    dx0 = rn(B, K) if want in ("dx", "all") else None
    stride = C + 7 if which == "dw_stride" else 0
    scale = 1.0 if affine else 0.625
    d_dy = torch.full((B, stride or C), NAN, dtype=torch.float32)
    d_dy[:, :C] = dy.float()
    d_dy, ddw, ddb, ddx = d_dy.to(dev()), f32(dw0), f32(db0), f32(dx0)
    dxk, dwk = f32(x), f32(w)
    _lib.check(_lib.lib().fg_op_linear_backward(int(affine), d_dy.data_ptr(), dxk.data_ptr(), dwk.data_ptr(), ptr(ddw), ptr(ddb), ptr(ddx), B, C, K,
                                                scale, stride, None))
    ref = R.linear_backward(dy, x, w, dw0, db0, dx0, scale)
    for name, t in (("dw", ddw), ("db", ddb), ("dx", ddx)):
        if t is not None:
            check(f"linear_backward fp32 {B}-{C}-{K}-{which} {name}", back(t), *ref[name])


@pytest.mark.parametrize("cout,cin,cin_pad,taps", [(128, 64, 256, 9), (256, 384, 512, 9), (128, 256, 256, 1), (24, 8, 256, 9)])
def test_dgrad_weights(cout, cin, cin_pad, taps):
    """fg_op_dgrad_weights -> launch_dgrad_weights: bit-identical to the flipped transpose, exact zeros in the rows from cin on."""
    w = torch.randn(cout, cin, taps, generator=torch.Generator().manual_seed(cout + cin))
    wt = torch.full((cin_pad, cout, taps), NAN, dtype=torch.float32, device=dev())
    wd = w.to(dev())
    _lib.check(_lib.lib().fg_op_dgrad_weights(wd.data_ptr(), wt.data_ptr(), cout, cin, cin_pad, taps, None))
    torch.cuda.synchronize()
    got = wt.cpu()
    assert torch.equal(got, R.dgrad_weights(w, cin_pad))
    ks = int(math.isqrt(taps))
    assert torch.equal(got[:cin], w.reshape(cout, cin, ks, ks).flip(-1, -2).transpose(0, 1).reshape(cin, cout, taps))
    assert (got[cin:] == 0).all()


# ---- elementwise pieces -----------------------------------------------------------------------------------------------------------------

OPS = {n: getattr(_lib, "FG_TRAIN_OP_" + n) for n in ("HEAD_GRAD", "STEM_OPERAND", "INPUT_GRAD", "ADD_NCHW_TO_NHWC", "SILU_BWD", "JVP_COEF",
                                                       "JVP_EMBED", "JVP_INPUT", "JVP_OUTPUT")}


def elementwise(op, dtype, a, b, c, d, e, out, batch, ch, ch_pad, hw, f0=0.0, f1=0.0, flag=0):
    _lib.check(_lib.lib().fg_op_train_elementwise(OPS[op], dtype, ptr(a), ptr(b), ptr(c), ptr(d), ptr(e), out.data_ptr(), batch, ch, ch_pad, hw, f0,
                                                  f1, flag, None))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("hw", [64, 1024])
@pytest.mark.parametrize("Cp", [8, 32])
def test_image_pieces(Cp, hw, B, dtype):
    """head_grad / stem_operand / input_grad / add_nchw_to_nhwc / jvp_input / jvp_output at C = 3 padded to Cp: padding channels exactly zero."""
    C = 3
    g = torch.Generator().manual_seed(Cp + hw + B)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64).float().to(F64)
    tag = f"{DT_NAME[dtype]} {Cp}-{hw}-{B}"
    src, coef = rn(B, C, hw), rn(B)
    for op in ("HEAD_GRAD", "STEM_OPERAND"):
        out = torch.full((B, hw, Cp), NAN, dtype=tdt(dtype), device=dev())
        elementwise(op, dtype, f32(src), f32(coef), None, None, None, out, B, C, Cp, hw)
        got = back(out)
        assert (got[..., C:] == 0).all()
        check(f"{op.lower()} {tag} out", got, *R.scaled_to_nhwc(src, coef, Cp, dtype))
    da, c_skip, dout = R.as_storage(rn(B, hw, C), dtype), rn(B), rn(B, C, hw)
    for with_skip in (False, True):
        out = torch.full((B, C, hw), NAN, dtype=torch.float32, device=dev())
        elementwise("INPUT_GRAD", dtype, pitched(da, Cp, dtype), f32(coef), f32(c_skip) if with_skip else None, f32(dout) if with_skip else None, None,
                    out, B, C, Cp, hw)
        check(f"input_grad {tag} skip{int(with_skip)}", back(out), *R.input_grad(da, coef, c_skip, dout if with_skip else None))
    dst = R.as_storage(rn(B, hw, Cp), dtype)
    srcp = rn(B, Cp, hw)
    dd = act(dst, dtype)
    elementwise("ADD_NCHW_TO_NHWC", dtype, f32(srcp), None, None, None, None, dd, B, Cp, Cp, hw)
    check(f"add_nchw_to_nhwc {tag} out", back(dd), *R.add_nchw_to_nhwc(srcp, dst, dtype))
    vx, x, dc_in = rn(B, C, hw), rn(B, C, hw), rn(B)
    out = torch.full((B, C, hw), NAN, dtype=torch.float32, device=dev())
    elementwise("JVP_INPUT", dtype, f32(vx), f32(x), f32(coef), f32(dc_in), None, out, B, C, Cp, hw)
    check(f"jvp_input {tag} out", back(out), *R.jvp_input(vx, x, coef, dc_in))
    fd, F_raw, ct = R.as_storage(rn(B, hw, C), dtype), rn(B, C, hw), rn(8, B)
    out = torch.full((B, C, hw), NAN, dtype=torch.float32, device=dev())
    elementwise("JVP_OUTPUT", dtype, pitched(fd, Cp, dtype), f32(F_raw), f32(x), f32(vx), f32(ct), out, B, C, Cp, hw)
    check(f"jvp_output {tag} out", back(out), *R.jvp_output(fd, F_raw, x, vx, ct))


@pytest.mark.parametrize("B,E", [(1, 8), (5, 512), (300, 3)])
def test_silu_bwd(B, E):
    g = torch.Generator().manual_seed(B + E)
    dy = torch.randn(B, E, generator=g, dtype=F64).float().to(F64)
    pre = (4.0 * torch.randn(B, E, generator=g, dtype=F64)).float().to(F64)
    pre[0, :3] = torch.tensor([0.0, -1.2784645, 30.0]).float().to(F64)  # 0, the zero of silu', a saturated sigmoid
    out = torch.full((B, E), NAN, dtype=torch.float32, device=dev())
    elementwise("SILU_BWD", 0, f32(dy), f32(pre), None, None, None, out, B, E, E, 1)
    check(f"silu_bwd fp32 {B}-{E} out", back(out), *R.silu_bwd(dy, pre))


@pytest.mark.parametrize("drop", [0, 1, 2, 3])
@pytest.mark.parametrize("with_r", [False, True])
def test_jvp_coef(drop, with_r):
    """jvp_coef_kernel against an fp64 evaluation of the preconditioning coefficients and their t-derivatives, t at both ends of the schedule."""
    t = torch.tensor([0.002, 80.0, 0.5, 1.0, 2.5e-7, 14.6], dtype=F64)
    r = torch.tensor([0.002, 40.0, 0.1, 5e-7, 1.0, 3.0], dtype=F64) if with_r else None
    B = t.numel()
    g = torch.Generator().manual_seed(drop)
    vt, vr = (torch.randn(B, generator=g, dtype=F64).float().to(F64) for _ in range(2))
    out = torch.full((8, B), NAN, dtype=torch.float32, device=dev())
    td, rd = t.to(dev()), None if r is None else r.to(dev())
    elementwise("JVP_COEF", 0, td, rd, f32(vt), f32(vr) if with_r else None, None, out, B, 0, 0, 0, 0.5, 0.25, drop)
    check(f"jvp_coef fp32 drop{drop}-r{int(with_r)} out", back(out), *R.jvp_coef(t, r, vt, vr if with_r else None, 0.5, 0.25, drop))


@pytest.mark.parametrize("B,N,noise_ch", [(1, 128, 128), (5, 256, 128), (3, 32, 16)])
def test_jvp_embed(B, N, noise_ch):
    g = torch.Generator().manual_seed(B + N)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64).float().to(F64)
    c_noise, r_noise, dc, dr = 2.0 * rn(B), 2.0 * rn(B), rn(B), rn(B)
    half = noise_ch // 2
    freqs = ((1.0 / 10000.0) ** (torch.arange(half, dtype=F64) / half)).float().to(F64)
    out = torch.full((B, N), NAN, dtype=torch.float32, device=dev())
    elementwise("JVP_EMBED", 0, f32(c_noise), f32(r_noise), f32(dc), f32(dr), f32(freqs), out, B, N, noise_ch, 1)
    check(f"jvp_embed fp32 {B}-{N}-{noise_ch} out", back(out), *R.jvp_embed(c_noise, r_noise, dc, dr, freqs, N, noise_ch))
