"""Plain fp64 references of the EDM training kernels (fastgen_amd/csrc/bwd.hip, attn_bwd.hip), written from the formulas in the two
files' header comments - never through autograd - each returning (value, bound): `bound` is a per-element, first-order bound of what
the kernel's own arithmetic may differ from `value` by.

How a bound is built.  Every stage of a kernel contributes u (n + 2) sum|terms| of its own sum (n terms, any order), u = 2^-24 for fp32
arithmetic (the bf16x3 GEMMs of nt_gemm_kernel<float> are exact-fp32 MFMA, so they take the same u); v_exp / v_rcp / expf / division add
a few u of the result; the errors of earlier stages are carried through the later ones to first order (|d f / d x| dx, summed in
absolute value).  `dtype` is the storage type of the activation tensors: 0 fp32, 1 bf16.

bf16 stores.  Rounding to bf16 (8 significant bits) is off by at most half an ulp, 2^(e - 9) for 2^(e - 1) <= |v| < 2^e: between
2^-9 |v| and 2^-8 |v|.  (2^-9 |v| itself is not a bound: 1 + 2^-8 - 2^-20 rounds to 1, off by 0.997 * 2^-8 |v|.)  The exact half ulp
is used.  Where a kernel stores an INTERMEDIATE in bf16 (P, dS and the transposes of the attention) the reference rounds there too,
and the carried error becomes the size of a rounding flip, charged only to the elements whose value lies within the carried error of
a rounding tie (`stored`); the final store of an output adds its half ulp (`final`).  Inputs of dtype 1 are bf16 values already.

`mut` selects a named mutation of a reference (GN_MUTATIONS, ATTN_MUTATIONS; "batch_ge4_dropped" of batchsum_add, "no_tap_flip" of
dgrad_weights): what a subtly wrong kernel would compute.  The CPU tests show that on the
GPU tests' inputs each mutation moves at least one element by more than the bound."""
import math

import torch

U = 2.0 ** -24
F64 = torch.float64

GN_MUTATIONS = ("no_s2", "octet_g0", "rm1_no_quarter", "rm2_three", "batch_ge4_dropped", "stats_image0", "mask_shift_octet")
ATTN_MUTATIONS = ("dk_from_ds", "softmax_first_wave", "dv_untransposed", "jvp_no_pvd")


def bf16_round(v):
    return v.to(torch.float32).to(torch.bfloat16).to(F64)  # values here are far inside fp32's range: the first cast does not double-round visibly


def hulp_bf16(v):
    """Half an ulp of bf16 at |v| (0 at 0)."""
    _, e = torch.frexp(v.abs().to(F64))
    return torch.where(v == 0, torch.zeros_like(v, dtype=F64), torch.ldexp(torch.ones_like(v, dtype=F64), e - 9))


def final(v, err, dtype):
    """Bound after the last store of an output whose exact value is v and carried error err."""
    if dtype == 0:
        return err + U * v.abs()
    return err + hulp_bf16(v.abs() + err)


def stored(v, err, dtype):
    """An intermediate the kernel stores in the storage type: (what the reference carries on, its error)."""
    if dtype == 0:
        return v, err + U * v.abs()
    r = bf16_round(v)
    h = hulp_bf16(v.abs() + err)
    tie = h - (v - r).abs()  # distance of v to the nearest rounding tie
    return r, torch.where(tie <= err, 4.0 * h + err, torch.zeros_like(err))  # a flip moves the stored value by one ulp (two at a binade edge)


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------

def gn_geometry(C):
    groups = min(32, C // 4)
    return groups, C // groups


def gn_coef(x, gamma, beta, eps, mut=None):
    """x [B, HW, C] fp64 -> dict of per-(image, channel) mean, rstd, a, b [B, 1, C] and their error bounds (gn_coeffs_kernel: fp32 partial
    sums of x and x^2 over ceil(HW / lanes) pixels x 4 channels, combined in fp64, mean and rstd rounded to fp32)."""
    B, HW, C = x.shape
    G, cpg = gn_geometry(C)
    xg = x.reshape(B, HW, G, cpg)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    ex2 = (xg ** 2).mean((1, 3))
    lanes = 512 // (C // 4)
    n = 4 * math.ceil(HW / lanes)
    dmean = U * (n + 2) * xg.abs().mean((1, 3)) + U * mean.abs()
    dvar = U * (n + 3) * ex2 + 2 * mean.abs() * dmean
    rstd = (var + eps) ** -0.5
    rho = 0.5 * dvar / (var + eps) + 2 * U  # relative error of rstd
    if mut == "stats_image0":
        mean, rstd = mean[:1].expand(B, G), rstd[:1].expand(B, G)
    ch = lambda t: t.repeat_interleave(cpg, 1)[:, None, :]
    mean, rstd, dmean, rho = ch(mean), ch(rstd), ch(dmean), ch(rho)
    a = rstd * gamma
    b = beta - a * mean
    da = a.abs() * (rho + U)
    db = mean.abs() * da + a.abs() * dmean + U * (b.abs() + (a * mean).abs())
    return dict(mean=mean, rstd=rstd, a=a, b=b, dmean=dmean, rho=rho, da=da, db=db, G=G, cpg=cpg)


def _sigmoid(y):
    return 1.0 / (1.0 + torch.exp(-y))


def _sigmoid_err(y, s):
    """Error of s = 1 / (1 + exp(-y)) as the kernels evaluate it.  The fast form is v_exp_f32 of the rounded product y * log2(e): the
    exponent moves by u |y| log2(e), i.e. e by u |y| relatively; v_exp adds one ulp, the sum and v_rcp one each (expf and a division
    are no worse); d s / d e = -s (1 - s) / e.  The last term is the rounding of s itself."""
    return s * (1 - s) * U * (y.abs() + 2) + U * s


def _silu_grad(y):
    """(silu'(y) = s (1 + y (1 - s)), the error of its evaluation s * fma(y, 1 - s, 1) at an exact y): the error of s enters through
    d silu' / d s = 1 + y (1 - 2 s) - for large y the rounding of s alone is |y| u - and the fma and the product add theirs."""
    s = _sigmoid(y)
    return s * (1 + y * (1 - s)), (1 + y * (1 - 2 * s)).abs() * _sigmoid_err(y, s) + 3 * U * s * (1 + y.abs() * (1 - s))


def _res_to_input(t, rm, mut=None):
    """A tensor at the conv's OUTPUT resolution [B, ro, ro, C] brought to the norm's (input) resolution (fetch_res): (value, sum of
    magnitudes of the terms added)."""
    if rm == 0:
        return t, torch.zeros_like(t)
    if rm == 1:  # the forward averaged 2x2: a quarter of the coarse value
        v = t.repeat_interleave(2, 1).repeat_interleave(2, 2)
        return (v if mut == "rm1_no_quarter" else 0.25 * v), torch.zeros_like(v)
    parts = [t[:, 0::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 0::2], t[:, 1::2, 1::2]]
    if mut == "rm2_three":
        parts = parts[:3]
    return sum(parts), sum(p.abs() for p in parts)


def _keep(keep, shape, mut=None):
    if keep is None:
        return torch.ones(shape, dtype=F64)
    k = keep.to(F64).reshape(shape)
    if mut == "mask_shift_octet":
        k = torch.roll(k.reshape(-1), 8).reshape(shape)
    return k


def gn_act(x, gamma, beta, eps, mode, rm, keep, dtype, mut=None):
    """gn_act_kernel: x [B, ri, ri, C] (the concat) -> out [B, res, res, C]; mode 0 silu(a x + b), 1 a x + b, 2 x; rm 1: mean of 2x2,
    rm 2: nearest 2x; keep (None or [B, res, res, C]) the dropout factors."""
    B, ri, _, C = x.shape
    if mode == 2:
        t, dt = x, torch.zeros_like(x)
    else:
        k = gn_coef(x.reshape(B, ri * ri, C), gamma, beta, eps)
        a, b, da, db = (k[n][:, :, None, :] for n in ("a", "b", "da", "db"))
        y = a * x + b
        dy = x.abs() * da + db + U * ((a * x).abs() + b.abs())
        if mode == 0:
            s = _sigmoid(y)
            t = y * s
            dt = (s * (1 + y.abs() * (1 - s))) * dy + y.abs() * _sigmoid_err(y, s) + 2 * U * t.abs()  # |silu'| dy, the sigmoid, the product
        else:
            t, dt = y, dy
    if rm == 1:
        parts = [t[:, 0::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 0::2], t[:, 1::2, 1::2]]
        eparts = [dt[:, 0::2, 0::2], dt[:, 0::2, 1::2], dt[:, 1::2, 0::2], dt[:, 1::2, 1::2]]
        t = 0.25 * sum(parts)
        dt = 0.25 * (sum(eparts) + 5 * U * sum(p.abs() for p in parts))
    elif rm == 2:
        t, dt = (v.repeat_interleave(2, 1).repeat_interleave(2, 2) for v in (t, dt))
    kf = _keep(keep, t.shape, mut)
    t, dt = t * kf, dt * kf + U * (t * kf).abs()
    return t, final(t, dt, dtype)


def gn_backward(x, dact, gamma, beta, eps, mode, rm, keep, add, add_scale, old, dtype, dg_old=None, db_old=None, mut=None):
    """launch_gn_bwd on x [B, res, res, C], dact (and add) at the conv's output resolution, channels [0, C) only.  old: the prior content
    of dx with `accumulate`, else None.  Returns {"dx": (v, bound), "dgamma": ..., "dbeta": ...} (the parameter gradients added to
    dg_old / db_old [C])."""
    B, res, _, C = x.shape
    HW = res * res
    k = gn_coef(x.reshape(B, HW, C), gamma, beta, eps, mut)
    G, cpg = k["G"], k["cpg"]
    sh = lambda t: t[:, :, None, :]
    mean, rstd, a, b, dmean, rho, da, db = (sh(k[n]) for n in ("mean", "rstd", "a", "b", "dmean", "rho", "da", "db"))
    dv, dvm = _res_to_input(dact, rm, mut)
    ddv = 4 * U * dvm
    kf = _keep(keep, x.shape, mut)
    dv, ddv = dv * kf, ddv * kf + (0 if keep is None else U) * (dv * kf).abs()
    xhat = (x - mean) * rstd
    dxhat = xhat.abs() * (rho + 3 * U) + rstd * dmean
    if mode == 0:
        y = a * x + b
        dy_ = x.abs() * da + db + U * ((a * x).abs() + b.abs())
        g, ge = _silu_grad(y)
        dg = 0.5 * dy_ + ge  # |silu''| <= 1/2
        dy = dv * g
        ddy = dv.abs() * dg + g.abs() * ddv + U * dy.abs()
    else:
        dy, ddy = dv, ddv
    n_pix = math.ceil(HW / 32) + 32  # a lane's chain, then the 32 lanes
    P1 = dy.sum((1, 2))
    P2 = (dy * xhat).sum((1, 2))
    dP1 = ddy.sum((1, 2)) + U * (n_pix + 2) * dy.abs().sum((1, 2))
    dP2 = (ddy * xhat.abs() + dy.abs() * dxhat).sum((1, 2)) + U * (n_pix + 3) * (dy * xhat).abs().sum((1, 2))
    out = {}
    n_b = math.ceil(B / 4) + 4
    Pb1, Pb2, dPb1, dPb2 = (P1, P2, dP1, dP2) if mut != "batch_ge4_dropped" else (P1[:4], P2[:4], dP1[:4], dP2[:4])
    for name, Pn, dPn, prior in (("dgamma", Pb2, dPb2, dg_old), ("dbeta", Pb1, dPb1, db_old)):
        if prior is not None:
            v = prior + Pn.sum(0)
            out[name] = (v, dPn.sum(0) + U * (n_b + 2) * (Pn.abs().sum(0) + prior.abs()))
    grp = lambda t: t.reshape(B, G, cpg).sum(2).repeat_interleave(cpg, 1)[:, None, None, :]
    S1, S2 = grp(gamma * P1), grp(gamma * P2)
    dS1 = grp(gamma.abs() * dP1 + U * (cpg + 2) * (gamma * P1).abs())
    dS2 = grp(gamma.abs() * dP2 + U * (cpg + 2) * (gamma * P2).abs())
    if mut == "octet_g0":  # the upper channels of an octet that straddles two groups read the lower group's statistics and sums
        c = torch.arange(C)
        src = torch.where((c // cpg) != ((c // 8) * 8) // cpg, ((c // 8) * 8), c)
        mean_, rstd_ = mean.expand(B, 1, 1, C)[..., src], rstd.expand(B, 1, 1, C)[..., src]
        S1, S2 = S1[..., src], S2[..., src]
        xhat = (x - mean_) * rstd_
        rstd = rstd_
    m = float(cpg * HW)
    s2 = 0.0 if mut == "no_s2" else 1.0
    core = rstd * (S1 + s2 * xhat * S2) / m
    v = a * dy - core
    err = (dy.abs() * da + a.abs() * ddy + (rstd / m) * (dS1 + xhat.abs() * dS2 + S2.abs() * dxhat) + (rho + 4 * U) * (rstd / m) * (S1.abs() + (xhat * S2).abs())
           + 2 * U * (a * dy).abs() + U * v.abs())
    if add is not None:
        av, avm = _res_to_input(add, rm, mut)
        v = v + add_scale * av
        err = err + abs(add_scale) * 4 * U * avm + 2 * U * (add_scale * av).abs() + U * v.abs()
    if old is not None:
        v = v + old
        err = err + U * v.abs()
    out["dx"] = (v, final(v, err, dtype))
    return out


def gn_jvp(x, xd, gamma, beta, eps, mode, keep, dtype, mut=None):
    """launch_gn_jvp: yd = a (xd - (S1 + xhat S2) / m) with the UNWEIGHTED group sums of {sum_p xd, sum_p xd xhat}; mode 0: * silu'(a x + b)."""
    B, res, _, C = x.shape
    HW = res * res
    k = gn_coef(x.reshape(B, HW, C), gamma, beta, eps, mut)
    G, cpg = k["G"], k["cpg"]
    sh = lambda t: t[:, :, None, :]
    mean, rstd, a, b, dmean, rho, da, db = (sh(k[n]) for n in ("mean", "rstd", "a", "b", "dmean", "rho", "da", "db"))
    xhat = (x - mean) * rstd
    dxhat = xhat.abs() * (rho + 3 * U) + rstd * dmean
    n_pix = math.ceil(HW / 32) + 32
    P1, P2 = xd.sum((1, 2)), (xd * xhat).sum((1, 2))
    dP1 = U * (n_pix + 2) * xd.abs().sum((1, 2))
    dP2 = (xd.abs() * dxhat).sum((1, 2)) + U * (n_pix + 3) * (xd * xhat).abs().sum((1, 2))
    grp = lambda t: t.reshape(B, G, cpg).sum(2).repeat_interleave(cpg, 1)[:, None, None, :]
    S1, S2 = grp(P1), grp(P2)
    dS1, dS2 = grp(dP1 + U * (cpg + 2) * P1.abs()), grp(dP2 + U * (cpg + 2) * P2.abs())
    if mut == "octet_g0":
        c = torch.arange(C)
        src = torch.where((c // cpg) != ((c // 8) * 8) // cpg, ((c // 8) * 8), c)
        S1, S2 = S1[..., src], S2[..., src]
        xhat = (x - mean.expand(B, 1, 1, C)[..., src]) * rstd.expand(B, 1, 1, C)[..., src]
    m = float(cpg * HW)
    s2 = 0.0 if mut == "no_s2" else 1.0
    inner = xd - (S1 + s2 * xhat * S2) / m
    dinner = (dS1 + xhat.abs() * dS2 + S2.abs() * dxhat) / m + 4 * U * (xd.abs() + (S1.abs() + (xhat * S2).abs()) / m)
    v = a * inner
    err = inner.abs() * da + a.abs() * dinner + U * v.abs()
    if mode == 0:
        y = a * x + b
        dy_ = x.abs() * da + db + U * ((a * x).abs() + b.abs())
        g, ge = _silu_grad(y)
        err = err * g.abs() + v.abs() * (0.5 * dy_ + ge) + U * (v * g).abs()
        v = v * g
    kf = _keep(keep, x.shape, mut)
    v, err = v * kf, err * kf + U * (v * kf).abs()
    return v, final(v, err, dtype)


# ---- attention ------------------------------------------------------------------------------------------------------------------

def _softmax_stage(q, k, dtype, mut=None):
    """P = softmax_rows(q k^T / sqrt(C)) as the kernels leave it in the storage type: (P, its error)."""
    T, C = q.shape[-2], q.shape[-1]
    sc = float(torch.tensor(1.0 / math.sqrt(C), dtype=torch.float32))
    s = sc * (q @ k.transpose(-1, -2))
    ds = sc * U * (C + 2) * (q.abs() @ k.abs().transpose(-1, -2)) + 2 * U * s.abs()
    e = torch.exp(s - s.amax(-1, keepdim=True))
    den = e[..., :64].sum(-1, keepdim=True) if mut == "softmax_first_wave" else e.sum(-1, keepdim=True)
    P = e / den
    dsm = ds.amax(-1, keepdim=True)  # the row maximum carries its own logit's error
    dP = P * (ds + dsm + (P * (ds + dsm)).sum(-1, keepdim=True) + 2 * U * (s - s.amax(-1, keepdim=True)).abs() + 16 * U)
    return stored(P, dP, dtype) + (sc,)


def _ds_stage(P, dP, g, dg, dtype):
    """attn_ds_kernel: P o (g - rowsum(P o g)) stored in the storage type."""
    d = (P * g).sum(-1, keepdim=True)
    dd = (dP * g.abs() + P * dg).sum(-1, keepdim=True) + 12 * U * (P * g).abs().sum(-1, keepdim=True)
    v = P * (g - d)
    err = dP * (g - d).abs() + P * (dg + dd + U * (g.abs() + d.abs())) + U * v.abs()
    return stored(v, err, dtype)


def attention_backward(q, k, vt, dO, dtype, mut=None):
    """launch_attention_backward: q, k, dO [B, T, C], vt [B, C, T] -> {"dq", "dk", "dvt"}: (value, bound)."""
    T, C = q.shape[-2], q.shape[-1]
    P, dP, sc = _softmax_stage(q, k, dtype, mut)
    g = dO @ vt  # dP[q][k] = sum_c dO[q][c] v[k][c]
    dg = U * (C + 2) * (dO.abs() @ vt.abs())
    dS, ddS = _ds_stage(P, dP, g, dg, dtype)
    tr = lambda t: t.transpose(-1, -2)
    out = {}
    for name, lhs, dlhs, rhs in (("dq", dS, ddS, k), ("dk", dS if mut == "dk_from_ds" else tr(dS), tr(ddS), q)):
        v = sc * (lhs @ rhs)
        err = sc * (dlhs @ rhs.abs() + U * (T + 2) * (lhs.abs() @ rhs.abs())) + 2 * U * v.abs()
        out[name] = (v, final(v, err, dtype))
    v = tr(dO) @ P  # dv^T[c][k] = sum_q dO[q][c] P[q][k]
    err = tr(dO).abs() @ dP + U * (T + 2) * (tr(dO).abs() @ P)
    if mut == "dv_untransposed":
        v = tr(v).reshape(v.shape)
    out["dvt"] = (v, final(v, err, dtype))
    return out


def attention_jvp(q, k, vt, qd, kd, vtd, dtype, mut=None):
    """launch_attention_jvp: Sd = (qd k^T + q kd^T) / sqrt(C), Pd = P o (Sd - rowsum(P o Sd)), od = Pd v + P vd."""
    T, C = q.shape[-2], q.shape[-1]
    P, dP, sc = _softmax_stage(q, k, dtype, mut)
    tr = lambda t: t.transpose(-1, -2)
    s1, s2 = sc * (qd @ tr(k)), sc * (q @ tr(kd))
    Sd = s1 + s2
    dSd = sc * U * (C + 2) * (qd.abs() @ tr(k).abs() + q.abs() @ tr(kd).abs()) + 2 * U * (s1.abs() + s2.abs()) + U * Sd.abs()
    Pd, dPd = _ds_stage(P, dP, Sd, dSd, dtype)
    o0, o1 = Pd @ tr(vt), P @ tr(vtd)
    e0 = dPd @ tr(vt).abs() + U * (T + 2) * (Pd.abs() @ tr(vt).abs())
    e1 = dP @ tr(vtd).abs() + U * (T + 2) * (P @ tr(vtd).abs())
    if mut == "jvp_no_pvd":
        o1 = torch.zeros_like(o1)
    v = o0 + o1
    return v, final(v, e0 + e1 + U * v.abs(), dtype)


# ---- sums, linear layers, weights ----------------------------------------------------------------------------------------------------

def colsum(t, scale):
    """colsum_kernel: t [B, HW, C] -> scale * sum_p, [B, C] fp32."""
    n = math.ceil(t.shape[1] / 32) + 32
    v = scale * t.sum(1)
    return v, abs(scale) * U * (n + 2) * t.abs().sum(1) + 2 * U * v.abs()


def batchsum_add(inp, old, mut=None):
    """batchsum_add_kernel: old [C] + sum_n inp [B, C] (four batch lanes, then their fixed-order sum, then +=)."""
    if mut == "batch_ge4_dropped":
        inp = inp[:4]
    n = math.ceil(inp.shape[0] / 4) + 4
    v = old + inp.sum(0)
    return v, U * (n + 2) * (inp.abs().sum(0) + old.abs()) + U * v.abs()


def linear_backward(dy, x, w, dw_old, db_old, dx_old, scale=1.0):
    """dw[c][k] += scale sum_b dy[b][c] x[b][k]; db[c] += sum_b dy; dx[b][k] += sum_c dy[b][c] w[c][k] - each for the prior given."""
    B, C = dy.shape
    out = {}
    if dw_old is not None:
        acc = dy.t() @ x
        v = dw_old + scale * acc
        out["dw"] = (v, U * (B + 2) * abs(scale) * (dy.abs().t() @ x.abs()) + 2 * U * (scale * acc).abs() + U * v.abs())
    if db_old is not None:
        out["db"] = batchsum_add(dy, db_old)
    if dx_old is not None:
        acc = dy @ w
        v = dx_old + acc
        out["dx"] = (v, U * (C + 2) * (dy.abs() @ w.abs()) + U * v.abs())
    return out


def dgrad_weights(w, cin_pad, mut=None):
    """w [cout, cin, taps] -> wt [cin_pad, cout, taps] = w[co][ci][taps - 1 - tap], zero rows from cin on.  Exact."""
    cout, cin, taps = w.shape
    wt = torch.zeros(cin_pad, cout, taps, dtype=w.dtype)
    wt[:cin] = (w if mut == "no_tap_flip" else w.flip(-1)).transpose(0, 1)
    return wt


# ---- elementwise pieces of the whole-network passes ---------------------------------------------------------------------------------------

def _pad_nhwc(v, Cp):
    """[B, C, HW] -> [B, HW, Cp] with zero channels from C on."""
    B, C, HW = v.shape
    out = torch.zeros(B, HW, Cp, dtype=F64)
    out[..., :C] = v.transpose(1, 2)
    return out


def scaled_to_nhwc(src, coef, Cp, dtype):
    """head_grad_kernel / stem_operand_kernel: out[n][p][c] = coef[n] src[n][c][p], zero for c >= C.  src [B, C, HW]."""
    v = _pad_nhwc(coef[:, None, None] * src, Cp)
    return v, final(v, U * v.abs(), dtype)


def input_grad(da, c_in, c_skip, dout):
    """input_grad_kernel: da [B, HW, C] (activation storage), dout [B, C, HW] or None -> dx [B, C, HW] fp32."""
    t0 = c_in[:, None, None] * da.transpose(1, 2)
    v, err = t0, U * t0.abs()
    if dout is not None:
        t1 = c_skip[:, None, None] * dout
        v = t0 + t1
        err = U * (t0.abs() + t1.abs()) + U * v.abs()
    return v, err


def add_nchw_to_nhwc(src, dst, dtype):
    """dst [B, HW, C] (activation storage) += src [B, C, HW] fp32."""
    v = dst + src.transpose(1, 2)
    return v, final(v, U * v.abs(), dtype)


def silu_bwd(dy, pre):
    g, ge = _silu_grad(pre)
    v = dy * g
    return v, dy.abs() * ge + U * v.abs()


def jvp_coef(t, r, vt, vr, sigma_data, sigma_shift, drop):
    """jvp_coef_kernel: [8, B] = c_in, dc_in, dc_noise, dr_noise, c_skip, dc_skip, c_out, dc_out (fp64 arithmetic, one rounding to fp32)."""
    B = t.shape[0]
    z, one = torch.zeros(B, dtype=F64), torch.ones(B, dtype=F64)
    dv = z if vt is None else vt
    rv = z if r is None else r
    drv = z if (r is None or vr is None) else vr
    s2 = sigma_data ** 2
    if drop & 1:
        rows = [one, z, dv, drv]
    else:
        qq = s2 + t * t
        rows = [qq ** -0.5, -t / qq ** 1.5 * dv, torch.where(t > 1e-6, dv / (4 * t.clamp_min(1e-300)), z),
                torch.where(rv > 1e-6, drv / (4 * rv.clamp_min(1e-300)), z)]
    if drop & 2:
        rows += [z, z, one, z]
    else:
        ts = t - sigma_shift
        qq = ts * ts + s2
        rows += [s2 / qq, -2 * ts * s2 / qq ** 2 * dv, ts * sigma_data / qq.sqrt(), sigma_data * s2 / qq ** 1.5 * dv]
    v = torch.stack(rows)
    return v, (U + 2.0 ** -48) * v.abs()


def jvp_embed(c_noise, r_noise, dc, dr, freqs, N, noise_ch):
    """jvp_embed_kernel: tangent of [cos | sin](label * freqs) per label, [B, N]."""
    half = noise_ch // 2
    j = torch.arange(N)
    first = j < noise_ch
    lab = torch.where(first[None], c_noise[:, None], r_noise[:, None])
    dl = torch.where(first[None], dc[:, None], dr[:, None])
    jj = j % noise_ch
    f = freqs[jj % half][None]
    ang = lab * f
    trig = torch.where((jj < half)[None], torch.cos(ang), -torch.sin(ang))
    v = trig * f * dl
    return v, (U * ang.abs() + 4 * U) * (f * dl).abs() + 2 * U * v.abs()


def jvp_input(vx, x, c_in, dc_in):
    sh = (-1,) + (1,) * (x.dim() - 1)
    t0, t1 = c_in.reshape(sh) * vx, dc_in.reshape(sh) * x
    return t0 + t1, U * (t0.abs() + 2 * t1.abs())


def jvp_output(fd, F_raw, x, vx, ct):
    """jvp_output_kernel: fd [B, HW, C] (activation storage), F_raw / x / vx [B, C, HW], ct [8, B] -> jvp [B, C, HW]."""
    cs, dcs, co, dco = (ct[i][:, None, None] for i in (4, 5, 6, 7))
    terms = [co * fd.transpose(1, 2), dco * F_raw, cs * vx, dcs * x]
    v = sum(terms)
    return v, 3 * U * sum(t.abs() for t in terms)


# ---- the inputs of the per-op tests (shared by the GPU tests and the CPU tests of the bounds and mutations) ------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def as_storage(t, dtype):
    """fp64 values a tensor of the storage type holds exactly (inputs of dtype 1 are pre-rounded to bf16)."""
    return bf16_round(t) if dtype else t.to(torch.float32).to(F64)


# (c1, c2, res, batch, mode, rm, add, accumulate, dx2, dropout p, parameter gradients): x at `res`; dact / add at res (rm 0), res / 2
# (rm 1), 2 res (rm 2).  C 16 and 96: cpg 4 (96: the second 64-channel workgroup half empty); 256: cpg 8; 256 + 128: cpg 12, a group
# straddles the concat and octets straddle groups; 256 + 256: cpg 16.  res 4: 16 pixels < the 32 pixel lanes.  batch 5: a second image
# on batch lane 0.
GN_CASES = [
    (16, 0, 4, 1, 0, 0, False, False, False, 0.0, True),
    (16, 0, 8, 5, 0, 1, True, True, False, 0.3, True),
    (96, 0, 4, 3, 0, 2, True, False, False, 0.0, False),
    (96, 0, 16, 5, 1, 0, False, True, False, 0.3, True),
    (96, 0, 8, 1, 0, 0, True, False, False, 0.0, True),
    (256, 0, 8, 3, 0, 0, True, False, False, 0.3, True),
    (256, 0, 16, 1, 0, 1, False, False, False, 0.0, False),
    (256, 128, 4, 5, 0, 0, True, True, True, 0.0, True),
    (256, 128, 8, 3, 0, 2, False, False, False, 0.3, True),
    (256, 128, 16, 5, 1, 1, True, False, True, 0.0, True),
    (256, 256, 4, 3, 0, 1, False, True, False, 0.0, False),
    (256, 256, 8, 5, 0, 0, True, False, True, 0.3, True),
    (256, 256, 16, 1, 0, 2, False, False, False, 0.0, True),
]


def _gn_sweep():
    """Every (C, res, batch) of C in {16, 96, 256, 256 + 128, 256 + 256} x res in {4, 8, 16} x batch in {1, 3, 5}, the other arguments
    dealt over the grid so that for every C each rm occurs with each res and each batch, and add / accumulate / dx2 / dropout / the
    parameter gradients / mode 1 are each on and off."""
    out = []
    for ic, (c1, c2) in enumerate(((16, 0), (96, 0), (256, 0), (256, 128), (256, 256))):
        for ir, res in enumerate((4, 8, 16)):
            for ib, B in enumerate((1, 3, 5)):
                k = 3 * ir + ib + ic
                out.append((c1, c2, res, B, int(k % 4 == 3), (ir + ib + ic) % 3, (ir + ib) % 2 == 0, (ib + ic + (ir > 0)) % 2 == 1,
                            c2 > 0 and (ir + ib) % 2 == 1, 0.3 if k % 2 else 0.0, k % 5 != 2))
    return out


GN_SWEEP = [c for c in _gn_sweep() if c not in GN_CASES]
GN_EPS = 1e-6
DROP_BLOCK, DROP_SEED = 7, (1 << 40) + 12345  # a seed above 2^32: both key words of the Philox stream are used


def gn_out_res(res, rm):
    return res // 2 if rm == 1 else (2 * res if rm == 2 else res)


def gn_inputs(case, dtype, seed=0):
    """x [B, res, res, C], dact / add [B, ro, ro, C], xd, gamma (mixed signs, one zero), beta, old dx, prior dgamma / dbeta.  The last
    image of a batch is 1000 x larger, so a statistic read from another image's row shows."""
    c1, c2, res, B, mode, rm, add, acc, dx2, p, params = case
    C, ro = c1 + c2, gn_out_res(res, rm)
    g = _gen(1000 + seed + 17 * C + res + 3 * B)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x = rn(B, res, res, C) + 0.25 * rn(1, 1, 1, C)
    if B > 1:
        x[B - 1] *= 1000.0
    gamma = (1.0 + 0.5 * rn(C)) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    gamma[C // 2 + 1] = 0.0
    d = dict(x=as_storage(x, dtype), dact=as_storage(rn(B, ro, ro, C), dtype), xd=as_storage(rn(B, res, res, C), dtype),
             gamma=gamma.float().to(F64), beta=(0.3 * rn(C)).float().to(F64), add=as_storage(rn(B, ro, ro, C), dtype) if add else None,
             old=as_storage(rn(B, res, res, C), dtype) if acc else None, dg_old=rn(C).float().to(F64) if params else None,
             db_old=rn(C).float().to(F64) if params else None)
    return d


# (T, C, batch, family).  T 64: one wave per softmax row; T 64 with C 256: the JVP's C > T branch.
ATTN_CASES = [
    (64, 32, 1, "noise"), (64, 32, 3, "eqkeys"), (64, 32, 1, "q0"), (64, 256, 3, "noise"), (64, 256, 1, "peaked"),
    (256, 32, 3, "peaked"), (256, 32, 1, "q0"), (256, 256, 1, "noise"), (256, 256, 3, "eqkeys"),
]


def attn_inputs(case, dtype, seed=0):
    """q, k, dO, qd, kd [B, T, C]; vt, vtd [B, C, T].  noise: seeded noise; q0: q = 0 (P uniform, dS pure cancellation); peaked: q x 8 with
    the row maximum at key 0 (rows 0, 4, ..) and key T - 1 (rows 2, 6, ..); eqkeys: the last image has all-equal keys."""
    T, C, B, fam = case
    g = _gen(2000 + seed + T + 7 * C + B)
    # Cubed normal deviates: every element is non-zero, but a few large terms carry each dot product, so sum|terms| / |sum| stays near
    # 3 at 256 terms (12.8 for normal deviates) and the u (n + 2) sum|terms| of a 256-term product stays below 2^-12 of the result.
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64) ** 3
    q, k, dO, qd, kd = (rn(B, T, C) for _ in range(5))
    q, qd = q / 15.0, qd / 15.0  # E z^6 = 15: logits of unit variance
    vt, vtd = rn(B, C, T), rn(B, C, T)
    if fam == "q0":
        q = torch.zeros_like(q)
    elif fam == "peaked":  # logit 8 above the rest at key 0 / T - 1: P_max about 0.9
        d = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).to(F64)
        # every fourth row peaks at key 0, the rows two further at key T - 1, odd rows stay plain noise: a saturated row turns the
        # u (C + 2) bound of its logits into a relative error of 1 / (1 - P_max) times that in dS, which at C = 256 is above 2^-12
        i = torch.arange(T)
        sign = torch.where(i % 4 == 0, 1.0, torch.where(i % 4 == 2, -1.0, 0.0)).to(F64)[None, :, None]
        q = 8.0 * (0.1 * q + sign * d / math.sqrt(C))
        k = 0.25 * k
        k[:, 0], k[:, T - 1] = d, -d
    elif fam == "eqkeys":
        k[B - 1] = k[B - 1, :1]
    return {n: as_storage(v, dtype) for n, v in dict(q=q, k=k, vt=vt, dO=dO, qd=qd, kd=kd, vtd=vtd).items()}
