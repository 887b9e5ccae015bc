// fg_op_* entry points over the launchers of the EDM training kernels (bwd.hip, attn_bwd.hip): no engine handle, device pointers, a
// caller-provided workspace.  Each checks its arguments, refuses what the launcher cannot serve and then calls the launcher the
// engine itself calls (engine_train.inc), so a per-op test runs the production kernels.  Included by engine.hip.

namespace {

bool gn_groups_ok(int C, bool octets) {
    if (C < 16 || C > 2048 || (C % 4)) return false;
    const int groups = C / 4 < 32 ? C / 4 : 32;
    if (C % groups) return false;
    const int cpg = C / groups;
    if (cpg % 4) return false;                 // launch_gn_coeffs: a thread owns a channel quad of one group
    return !octets || cpg == 4 || cpg >= 8;    // load_oct_coef: an octet spans at most two groups
}
bool aligned16(const void* p) { return !(((uintptr_t)p) & 15); }

// workspace of the GroupNorm ops: ab [B][C], P [B][C], mr [B][32], S [B][32], all float2
struct GnWs {
    float2 *ab, *P, *mr, *S;
};
size_t gn_ws_bytes(int B, int C) { return (size_t)B * (2 * (size_t)C + 64) * sizeof(float2) + 256; }
GnWs gn_ws_cut(void* ws, int B, int C) {
    GnWs w;
    w.ab = (float2*)ws;
    w.P = w.ab + (size_t)B * C;
    w.mr = w.P + (size_t)B * C;
    w.S = w.mr + (size_t)B * 32;
    return w;
}

}  // namespace

size_t fg_op_gn_workspace_bytes(int batch, int c) { return batch > 0 && gn_groups_ok(c, false) ? gn_ws_bytes(batch, c) : 0; }

int fg_op_gn_act(int dtype, int mode, const void* x1, int c1, const void* x2, int c2, const float* gamma, const float* beta, float eps,
                 void* out, int batch, int res, int rm, float drop_p, uint32_t drop_block, uint64_t drop_seed, void* workspace,
                 size_t workspace_bytes, void* stream) {
    const int C = c1 + c2;
    if ((dtype != 0 && dtype != 1) || mode < 0 || mode > 2 || rm < 0 || rm > 2)
        return fail(FG_EINVAL, "fg_op_gn_act: dtype %d (0 fp32, 1 bf16), mode %d (0, 1, 2), rm %d (0, 1, 2)", dtype, mode, rm);
    if (c1 <= 0 || c2 < 0 || (c1 % 8) || (c2 % 8)) return fail(FG_EINVAL, "fg_op_gn_act: c1 %d > 0 and c2 %d >= 0 must be multiples of 8", c1, c2);
    if (batch <= 0 || batch > 65535 || res <= 0 || res > 1024 || (rm == 2 && (res & 1)))
        return fail(FG_EINVAL, "fg_op_gn_act: batch %d (1 .. 65535), res %d (1 .. 1024, even with rm 2)", batch, res);
    if (mode != 2 && !gn_groups_ok(C, false)) return fail(FG_EINVAL, "fg_op_gn_act: %d channels: no GroupNorm of groups that are multiples of 4", C);
    if (!(drop_p >= 0.f && drop_p < 1.f)) return fail(FG_EINVAL, "fg_op_gn_act: dropout p %g outside [0, 1)", (double)drop_p);
    if (!x1 || (c2 && !x2) || !out || (mode != 2 && (!gamma || !beta || !workspace))) return fail(FG_EINVAL, "fg_op_gn_act: null pointer");
    if (!aligned16(x1) || !aligned16(x2) || !aligned16(out) || !aligned16(workspace))
        return fail(FG_EINVAL, "fg_op_gn_act: x1 / x2 / out / workspace must be 16-byte aligned");
    GnWs w{};
    const int ri = rm == 1 ? res * 2 : (rm == 2 ? res / 2 : res);
    hipStream_t s = (hipStream_t)stream;
    if (mode != 2) {
        if (workspace_bytes < gn_ws_bytes(batch, C))
            return fail(FG_EINVAL, "fg_op_gn_act: workspace too small (%zu < %zu bytes)", workspace_bytes, gn_ws_bytes(batch, C));
        w = gn_ws_cut(workspace, batch, C);
        HIP_TRY(launch_gn_coeffs(dtype, x1, c1, c2 ? x2 : nullptr, c2, gamma, beta, eps, w.ab, batch, ri * ri, s, w.mr));
    }
    HIP_TRY(launch_gn_act(dtype, mode, x1, c1, c2 ? x2 : nullptr, c2, w.ab, out, batch, res, rm, s, DropArgs{drop_p, drop_block, drop_seed}));
    return FG_OK;
}

int fg_op_gn_backward(int dtype, int mode, const void* x1, int c1, const void* x2, int c2, const void* dact, int cd, const float* gamma,
                      const float* beta, float eps, float* dgamma, float* dbeta, const void* add, int ca, float add_scale, void* dx, void* dx2,
                      int accumulate, int batch, int res, int rm, float drop_p, uint32_t drop_block, uint64_t drop_seed, void* workspace,
                      size_t workspace_bytes, void* stream) {
    const int C = c1 + c2;
    if ((dtype != 0 && dtype != 1) || (mode != 0 && mode != 1) || rm < 0 || rm > 2)
        return fail(FG_EINVAL, "fg_op_gn_backward: dtype %d (0 fp32, 1 bf16), mode %d (0, 1), rm %d (0, 1, 2)", dtype, mode, rm);
    if (c1 <= 0 || c2 < 0 || (c1 % 8) || (c2 % 8)) return fail(FG_EINVAL, "fg_op_gn_backward: c1 %d > 0 and c2 %d >= 0 must be multiples of 8", c1, c2);
    if (!gn_groups_ok(C, true))
        return fail(FG_EINVAL, "fg_op_gn_backward: %d channels: the group size must be 4 or a multiple of 4 that is at least 8", C);
    if (batch <= 0 || batch > 65535 || res <= 0 || res > 1024 || (rm == 1 && (res & 1)))
        return fail(FG_EINVAL, "fg_op_gn_backward: batch %d (1 .. 65535), res %d (1 .. 1024, even with rm 1)", batch, res);
    if (cd < C || (cd % 8) || (add && (ca < C || (ca % 8))))
        return fail(FG_EINVAL, "fg_op_gn_backward: pitches cd %d and ca %d must be multiples of 8 and at least C = %d", cd, ca, C);
    if (!(drop_p >= 0.f && drop_p < 1.f)) return fail(FG_EINVAL, "fg_op_gn_backward: dropout p %g outside [0, 1)", (double)drop_p);
    if (!x1 || (c2 && !x2) || !dact || !gamma || !beta || !dx || !workspace) return fail(FG_EINVAL, "fg_op_gn_backward: null pointer");
    if (dx2 && !c2) return fail(FG_EINVAL, "fg_op_gn_backward: dx2 without a second source");
    if (!aligned16(x1) || !aligned16(x2) || !aligned16(dact) || !aligned16(add) || !aligned16(dx) || !aligned16(dx2) || !aligned16(workspace))
        return fail(FG_EINVAL, "fg_op_gn_backward: x1 / x2 / dact / add / dx / dx2 / workspace must be 16-byte aligned");
    if (workspace_bytes < gn_ws_bytes(batch, C))
        return fail(FG_EINVAL, "fg_op_gn_backward: workspace too small (%zu < %zu bytes)", workspace_bytes, gn_ws_bytes(batch, C));
    const GnWs w = gn_ws_cut(workspace, batch, C);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_gn_coeffs(dtype, x1, c1, c2 ? x2 : nullptr, c2, gamma, beta, eps, w.ab, batch, res * res, s, w.mr));
    HIP_TRY(launch_gn_bwd(dtype, mode, x1, c1, c2 ? x2 : nullptr, c2, dact, cd, w.ab, w.mr, gamma, w.P, w.S, dgamma, dbeta, add, ca, add_scale, dx,
                          batch, res, rm, s, dx2, accumulate, DropArgs{drop_p, drop_block, drop_seed}));
    return FG_OK;
}

int fg_op_gn_jvp(int dtype, int mode, const void* x1, int c1, const void* x2, int c2, const void* xd, const float* gamma, const float* beta,
                 float eps, void* out, int batch, int res, float drop_p, uint32_t drop_block, uint64_t drop_seed, void* workspace,
                 size_t workspace_bytes, void* stream) {
    const int C = c1 + c2;
    if ((dtype != 0 && dtype != 1) || (mode != 0 && mode != 1)) return fail(FG_EINVAL, "fg_op_gn_jvp: dtype %d (0 fp32, 1 bf16), mode %d (0, 1)", dtype, mode);
    if (c1 <= 0 || c2 < 0 || (c1 % 8) || (c2 % 8)) return fail(FG_EINVAL, "fg_op_gn_jvp: c1 %d > 0 and c2 %d >= 0 must be multiples of 8", c1, c2);
    if (!gn_groups_ok(C, true)) return fail(FG_EINVAL, "fg_op_gn_jvp: %d channels: the group size must be 4 or a multiple of 4 that is at least 8", C);
    if (batch <= 0 || batch > 65535 || res <= 0 || res > 1024) return fail(FG_EINVAL, "fg_op_gn_jvp: batch %d (1 .. 65535), res %d (1 .. 1024)", batch, res);
    if (!(drop_p >= 0.f && drop_p < 1.f)) return fail(FG_EINVAL, "fg_op_gn_jvp: dropout p %g outside [0, 1)", (double)drop_p);
    if (!x1 || (c2 && !x2) || !xd || !gamma || !beta || !out || !workspace) return fail(FG_EINVAL, "fg_op_gn_jvp: null pointer");
    if (!aligned16(x1) || !aligned16(x2) || !aligned16(xd) || !aligned16(out) || !aligned16(workspace))
        return fail(FG_EINVAL, "fg_op_gn_jvp: x1 / x2 / xd / out / workspace must be 16-byte aligned");
    if (workspace_bytes < gn_ws_bytes(batch, C))
        return fail(FG_EINVAL, "fg_op_gn_jvp: workspace too small (%zu < %zu bytes)", workspace_bytes, gn_ws_bytes(batch, C));
    const GnWs w = gn_ws_cut(workspace, batch, C);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_gn_coeffs(dtype, x1, c1, c2 ? x2 : nullptr, c2, gamma, beta, eps, w.ab, batch, res * res, s, w.mr));
    HIP_TRY(launch_gn_jvp(dtype, mode, x1, c1, c2 ? x2 : nullptr, c2, xd, w.ab, w.mr, w.P, w.S, out, batch, res, s,
                          DropArgs{drop_p, drop_block, drop_seed}));
    return FG_OK;
}

size_t fg_op_attention_backward_workspace_bytes(int dtype, int batch, int t, int c) {
    if ((dtype != 0 && dtype != 1) || batch <= 0 || batch > 65535 || (t != 64 && t != 256) || c <= 0 || (c % 32) || c > 4096) return 0;
    return attention_backward_scratch_bytes(dtype, batch, t, c);
}
namespace {
int attn_op_check(const char* name, int dtype, int batch, int t, int c, const void* workspace, size_t workspace_bytes) {
    const size_t need = fg_op_attention_backward_workspace_bytes(dtype, batch, t, c);
    if (!need) return fail(FG_EINVAL, "%s: unsupported dtype %d (0, 1), batch %d, t %d (64, 256) or c %d (a multiple of 32)", name, dtype, batch, t, c);
    if (!workspace || (((uintptr_t)workspace) & 255)) return fail(FG_EINVAL, "%s: the workspace must be 256-byte aligned", name);
    if (workspace_bytes < need) return fail(FG_EINVAL, "%s: workspace too small (%zu < %zu bytes)", name, workspace_bytes, need);
    return FG_OK;
}
}  // namespace
int fg_op_attention_backward(int dtype, const void* q, const void* k, const void* vt, const void* d_out, void* dq, void* dk, void* dvt,
                             void* dqkv, int batch, int t, int c, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int e = attn_op_check("fg_op_attention_backward", dtype, batch, t, c, workspace, workspace_bytes)) return e;
    if (!q || !k || !vt || !d_out || !dq || !dk || !dvt) return fail(FG_EINVAL, "fg_op_attention_backward: null pointer");
    if (!aligned16(q) || !aligned16(k) || !aligned16(vt) || !aligned16(d_out) || !aligned16(dq) || !aligned16(dk) || !aligned16(dvt))
        return fail(FG_EINVAL, "fg_op_attention_backward: tensors must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_attention_backward(dtype, q, k, vt, d_out, dq, dk, dvt, workspace, batch, t, c, s));
    if (dqkv) HIP_TRY(launch_qkv_interleave(dtype, dq, dk, dvt, dqkv, batch, t, c, s));
    return FG_OK;
}
int fg_op_attention_jvp(int dtype, const void* q, const void* k, const void* vt, const void* qd, const void* kd, const void* vtd, void* od,
                        int batch, int t, int c, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int e = attn_op_check("fg_op_attention_jvp", dtype, batch, t, c, workspace, workspace_bytes)) return e;
    if (!q || !k || !vt || !qd || !kd || !vtd || !od) return fail(FG_EINVAL, "fg_op_attention_jvp: null pointer");
    if (!aligned16(q) || !aligned16(k) || !aligned16(vt) || !aligned16(qd) || !aligned16(kd) || !aligned16(vtd) || !aligned16(od))
        return fail(FG_EINVAL, "fg_op_attention_jvp: tensors must be 16-byte aligned");
    HIP_TRY(launch_attention_jvp(dtype, q, k, vt, qd, kd, vtd, od, workspace, batch, t, c, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_colsum(int dtype, const void* t, int ct, int c, float* out, int batch, int hw, float scale, int out_stride, void* stream) {
    if ((dtype != 0 && dtype != 1) || c <= 0 || (c % 8) || ct < c || (ct % 8) || batch <= 0 || batch > 65535 || hw <= 0 || (out_stride && out_stride < c))
        return fail(FG_EINVAL, "fg_op_colsum: dtype %d (0, 1), c %d > 0 and ct %d >= c multiples of 8, batch %d (1 .. 65535), hw %d > 0, out_stride %d (0 or >= c)",
                    dtype, c, ct, batch, hw, out_stride);
    if (!t || !out || !aligned16(t)) return fail(FG_EINVAL, "fg_op_colsum: null or misaligned pointer");
    HIP_TRY(launch_colsum(dtype, t, ct, c, out, batch, hw, scale, (hipStream_t)stream, out_stride));
    return FG_OK;
}
int fg_op_batchsum_add(const float* in, float* out, float* out2, int batch, int c, int in_stride, void* stream) {
    if (batch <= 0 || c <= 0 || (in_stride && in_stride < c))
        return fail(FG_EINVAL, "fg_op_batchsum_add: batch %d > 0, c %d > 0, in_stride %d (0 or >= c)", batch, c, in_stride);
    if (!in || !out) return fail(FG_EINVAL, "fg_op_batchsum_add: null pointer");
    HIP_TRY(launch_batchsum_add(in, out, batch, c, (hipStream_t)stream, out2, in_stride));
    return FG_OK;
}

int fg_op_linear_backward(int affine, const float* dy, const float* x, const float* w, float* dw, float* db, float* dx, int batch, int c, int k,
                          float scale, int dy_stride, void* stream) {
    if (batch <= 0 || c <= 0 || k <= 0 || (int64_t)c * k > (1 << 30) || (int64_t)batch * k > (1 << 30))
        return fail(FG_EINVAL, "fg_op_linear_backward: batch %d, c %d, k %d must be positive, c k and batch k at most 2^30", batch, c, k);
    if (!dy || (dw && !x) || (dx && !w) || (!dw && !db && !dx)) return fail(FG_EINVAL, "fg_op_linear_backward: null pointer, or nothing to compute");
    hipStream_t s = (hipStream_t)stream;
    if (affine) {
        if (db || scale != 1.0f || (dy_stride && dy_stride != c))
            return fail(FG_EINVAL, "fg_op_linear_backward: the embedding-affine form has no bias gradient, scale or row stride");
        HIP_TRY(launch_affine_bwd(dy, x, w, dw, dx, batch, c, k, s));
        return FG_OK;
    }
    if (dy_stride && dy_stride < c) return fail(FG_EINVAL, "fg_op_linear_backward: dy_stride %d < c %d", dy_stride, c);
    if ((db || dx) && dy_stride && dy_stride != c) return fail(FG_EINVAL, "fg_op_linear_backward: only the weight gradient takes a row stride");
    HIP_TRY(launch_linear_bwd(dy, x, w, dw, db, dx, batch, c, k, scale, s, dy_stride));
    return FG_OK;
}

int fg_op_dgrad_weights(const float* w, float* wt, int cout, int cin, int cin_pad, int taps, void* stream) {
    if (cout <= 0 || cin <= 0 || cin_pad < cin || (taps != 1 && taps != 9) || (int64_t)cin_pad * cout * taps > ((int64_t)1 << 31))
        return fail(FG_EINVAL, "fg_op_dgrad_weights: cout %d > 0, cin %d > 0, cin_pad %d >= cin, taps %d (1, 9)", cout, cin, cin_pad, taps);
    if (!w || !wt) return fail(FG_EINVAL, "fg_op_dgrad_weights: null pointer");
    HIP_TRY(launch_dgrad_weights(w, wt, cout, cin, cin_pad, taps, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_train_elementwise(int op, int dtype, const void* a, const void* b, const void* c, const void* d, const void* e, void* out, int batch,
                            int ch, int ch_pad, int hw, double f0, double f1, int flag, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (dtype != 0 && dtype != 1) return fail(FG_EINVAL, "fg_op_train_elementwise: dtype %d (0 fp32, 1 bf16)", dtype);
    if (batch <= 0 || !out || !a) return fail(FG_EINVAL, "fg_op_train_elementwise: batch %d > 0, non-null a and out", batch);
    const bool img = ch > 0 && hw > 0 && (int64_t)batch * hw * (ch_pad > ch ? ch_pad : ch) < ((int64_t)1 << 40);
    switch (op) {
    case FG_TRAIN_OP_HEAD_GRAD:
    case FG_TRAIN_OP_STEM_OPERAND:
        if (!img || ch_pad < ch || !b) return fail(FG_EINVAL, "fg_op_train_elementwise: op %d needs ch %d > 0, ch_pad %d >= ch, hw %d > 0 and b", op, ch, ch_pad, hw);
        if (op == FG_TRAIN_OP_HEAD_GRAD)
            HIP_TRY(launch_head_grad(dtype, (const float*)a, (const float*)b, out, batch, ch, ch_pad, hw, s));
        else
            HIP_TRY(launch_stem_operand(dtype, (const float*)a, (const float*)b, out, batch, ch, ch_pad, hw, s));
        return FG_OK;
    case FG_TRAIN_OP_INPUT_GRAD:
        if (!img || ch_pad < ch || !b || (d && !c)) return fail(FG_EINVAL, "fg_op_train_elementwise: input_grad needs ch_pad >= ch, c_in (b) and c_skip (c) with dout (d)");
        HIP_TRY(launch_input_grad(dtype, a, ch_pad, (const float*)b, (const float*)c, (const float*)d, (float*)out, batch, ch, hw, s));
        return FG_OK;
    case FG_TRAIN_OP_ADD_NCHW_TO_NHWC:
        if (!img) return fail(FG_EINVAL, "fg_op_train_elementwise: add_nchw_to_nhwc needs ch %d > 0 and hw %d > 0", ch, hw);
        HIP_TRY(launch_add_nchw_to_nhwc(dtype, (const float*)a, out, batch, ch, hw, s));
        return FG_OK;
    case FG_TRAIN_OP_SILU_BWD:
        if (ch <= 0 || !b || (int64_t)batch * ch > (1 << 30)) return fail(FG_EINVAL, "fg_op_train_elementwise: silu_bwd needs ch %d > 0 and pre (b)", ch);
        HIP_TRY(launch_silu_bwd((const float*)a, (const float*)b, (float*)out, batch * ch, s));
        return FG_OK;
    case FG_TRAIN_OP_JVP_COEF:
        if (flag < 0 || flag > 3) return fail(FG_EINVAL, "fg_op_train_elementwise: jvp_coef drop mask %d (0 .. 3)", flag);
        HIP_TRY(launch_jvp_coef((const double*)a, (const double*)b, (const float*)c, (const float*)d, f0, f1, flag, (float*)out, batch, s));
        return FG_OK;
    case FG_TRAIN_OP_JVP_EMBED:
        // ch = N (width of the mapping input: noise_ch or 2 noise_ch), ch_pad = noise_ch
        if (ch_pad < 2 || (ch_pad & 1) || (ch != ch_pad && ch != 2 * ch_pad) || !b || !c || !d || !e)
            return fail(FG_EINVAL, "fg_op_train_elementwise: jvp_embed needs noise_ch %d even, n %d = noise_ch or 2 noise_ch and b, c, d, e", ch_pad, ch);
        HIP_TRY(launch_jvp_embed((const float*)a, (const float*)b, (const float*)c, (const float*)d, (const float*)e, (float*)out, batch, ch, ch_pad, s));
        return FG_OK;
    case FG_TRAIN_OP_JVP_INPUT:
        if (!img || !b || !c || !d) return fail(FG_EINVAL, "fg_op_train_elementwise: jvp_input needs ch, hw > 0 and b, c, d");
        HIP_TRY(launch_jvp_input((const float*)a, (const float*)b, (const float*)c, (const float*)d, (float*)out, batch, ch * hw, s));
        return FG_OK;
    case FG_TRAIN_OP_JVP_OUTPUT:
        if (!img || ch_pad < ch || !b || !c || !d || !e) return fail(FG_EINVAL, "fg_op_train_elementwise: jvp_output needs ch_pad >= ch and b, c, d, e");
        HIP_TRY(launch_jvp_output(dtype, a, ch_pad, (const float*)b, (const float*)c, (const float*)d, (const float*)e, (float*)out, batch, ch, hw, s));
        return FG_OK;
    default:
        return fail(FG_EINVAL, "fg_op_train_elementwise: unknown op %d", op);
    }
}
