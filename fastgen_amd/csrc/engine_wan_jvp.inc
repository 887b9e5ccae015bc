// Forward-mode derivative of the bidirectional video DiT (Wan.jvp; MeanFlow's tangent, reference
// fastgen/methods/consistency_model/mean_flow.py:220-252 - which, for this network, falls back to a finite difference because its flash
// attention has no forward-mode rule: configs/experiments/WanT2V/config_mf.py).  fg_wan_jvp runs fg_wan_forward_full's schedule on two
// bf16 token streams, primal x and tangent xd, with a schedule of its own (wan_forward / wan_block stay what they were): the
// non-GEMM pieces are wan_jvp.hip's, a tangent linear is wan_gemm on the tangent operand with the same packed weights and a null bias.
// Gated residual x' = x + g (W o + b):  xd' = xd + g (W od) + gd (W o + b) - the primal launch is the forward's, the tangent takes the
// same epilogue twice: once on od with gate g and a null bias, once on the primal operand o with gate gd on top of the first result.
// Textually included by engine.hip behind engine_wan.inc.
}  // extern "C" (reopened below)

namespace {

struct WanJvpWs {
    float *zrow, *zbias, *rrow, *rrowd;       // zero rows (null vt / vr, the tangent embedding's bias); the r_embedder's input rows
    float *tf, *tfd, *th, *thd, *e, *ed;      // fourier features, hidden layer, embedding (scratch of one embedder at a time)
    float *temb, *tembd, *st, *std_, *tproj, *tprojd, *rproj, *rprojd, *mod, *omod, *omodd;
    float2* cs;
    void *x[2], *xd[3];                       // the primal pair, the tangent triple (two GEMMs per gated residual)
    void *y, *yd, *qkv, *qkvd, *qn, *qnd, *kf, *kfd, *vf, *vfd, *att, *attd, *hid, *hidd;
    float* gs;
    size_t gs_bytes;
};

size_t wan_jvp_plan(const fg_wan* h, int B, int Fr, int gh, int gw, Arena& A, WanJvpWs& w) {
    const size_t D = h->D, BF = (size_t)B * Fr, M = BF * gh * gw, L = (size_t)Fr * gh * gw, fq = h->cfg.freq_dim;
    w.zrow = A.get<float>(BF);
    w.zbias = A.get<float>(D);
    w.rrow = A.get<float>(BF);
    w.rrowd = A.get<float>(BF);
    w.tf = A.get<float>(BF * fq), w.tfd = A.get<float>(BF * fq);
    w.th = A.get<float>(BF * D), w.thd = A.get<float>(BF * D);
    w.e = A.get<float>(BF * D), w.ed = A.get<float>(BF * D);
    w.temb = A.get<float>(BF * D), w.tembd = A.get<float>(BF * D);
    w.st = A.get<float>(BF * D), w.std_ = A.get<float>(BF * D);
    w.tproj = A.get<float>(BF * 6 * D), w.tprojd = A.get<float>(BF * 6 * D);
    w.rproj = A.get<float>(BF * 6 * D), w.rprojd = A.get<float>(BF * 6 * D);
    w.mod = A.get<float>(BF * 6 * D);
    w.omod = A.get<float>(BF * 2 * D), w.omodd = A.get<float>(BF * 2 * D);
    w.cs = A.get<float2>(L * 64);
    for (void*& p : w.x) p = A.take(M * D * 2);
    for (void*& p : w.xd) p = A.take(M * D * 2);
    w.y = A.take(M * D * 2), w.yd = A.take(M * D * 2);
    w.qkv = A.take(M * 3 * D * 2), w.qkvd = A.take(M * 3 * D * 2);
    w.qn = A.take(M * D * 2), w.qnd = A.take(M * D * 2);
    w.kf = A.take(M * D * 2), w.kfd = A.take(M * D * 2);
    w.vf = A.take(M * D * 2), w.vfd = A.take(M * D * 2);
    w.att = A.take(M * D * 2), w.attd = A.take(M * D * 2);
    w.hid = A.take(M * (size_t)h->Fd * 2), w.hidd = A.take(M * (size_t)h->Fd * 2);
    w.gs_bytes = 4 * M * D * 4;
    w.gs = (float*)A.take(w.gs_bytes);
    return (A.off + 255) & ~(size_t)255;
}

// FG_EINVAL on a handle that has no jvp
int wan_jvp_refusal(const fg_wan* h) {
    if (h->fp8) return fail(FG_EINVAL, "fg_wan_jvp: the fp8 compute mode has no forward-mode derivative (bf16 handles only)");
    if (const char* v = wan_variant(h)) return fail(FG_EINVAL, "fg_wan_jvp: not implemented for %s", v);
    return FG_OK;
}

// One time embedder with tangent: rows t / td -> embedding e / ed [BF][D] and projection p / pd [BF][6 D]
// (Timesteps -> Linear - SiLU - Linear, then time_proj(silu(.)); the tangent of a linear has no bias)
int wan_jvp_embedder(const fg_wan* h, const float* t, const float* td, int w1, int b1, int w2, int b2, int wp, int bp, float* e, float* ed, float* p,
                     float* pd, int BF, WanJvpWs& w, hipStream_t s) {
    const int D = h->D, fq = h->cfg.freq_dim;
    HIP_TRY(launch_dit_fourier_jvp(t, td, w.tf, w.tfd, BF, fq, s));
    HIP_TRY(launch_linear(w.tf, h->P(w1), h->P(b1), w.th, BF, fq, D, 0, s));
    HIP_TRY(launch_linear(w.tfd, h->P(w1), nullptr, w.thd, BF, fq, D, 0, s));
    HIP_TRY(launch_dit_silu_jvp(w.th, w.thd, nullptr, w.th, w.thd, BF * D, s));
    HIP_TRY(launch_linear(w.th, h->P(w2), h->P(b2), e, BF, D, D, 0, s));
    HIP_TRY(launch_linear(w.thd, h->P(w2), nullptr, ed, BF, D, D, 0, s));
    HIP_TRY(launch_dit_silu_jvp(e, ed, nullptr, w.st, w.std_, BF * D, s));
    HIP_TRY(launch_linear(w.st, h->P(wp), h->P(bp), p, BF, D, 6 * D, 0, s));
    HIP_TRY(launch_linear(w.std_, h->P(wp), nullptr, pd, BF, D, 6 * D, 0, s));
    return FG_OK;
}

// x' = x + g (a W^T + b) and its tangent (g == nullptr: no gate) on the stream pairs; x[0] / xd[0] are the streams before and after
int wan_jvp_residual(WanJvpWs& w, const void* a, const void* ad, const void* W, const float* bias, const float* g, const float* gd, int gstride,
                     int grows, int M, int N, int K, hipStream_t s) {
    int rc;
    if ((rc = wan_gemm(WanOperand{a}, W, bias, w.x[1], M, N, K, s, 0, g, gstride, grows, w.x[0], w.gs, w.gs_bytes)) ||
        (rc = wan_gemm(WanOperand{ad}, W, nullptr, w.xd[1], M, N, K, s, 0, g, gstride, grows, w.xd[0], w.gs, w.gs_bytes)))
        return rc;
    std::swap(w.x[0], w.x[1]);
    std::swap(w.xd[0], w.xd[1]);
    if (g) {
        if ((rc = wan_gemm(WanOperand{a}, W, bias, w.xd[2], M, N, K, s, 0, gd, gstride, grows, w.xd[0], w.gs, w.gs_bytes))) return rc;
        std::swap(w.xd[0], w.xd[2]);
    }
    return FG_OK;
}

int wan_jvp_block(fg_wan* h, fg_wan::Blk& b, WanJvpWs& w, int batch, int fs, int L, int M, int BF, hipStream_t s) {
    const fg_wan_config& c = h->cfg;
    const int D = h->D;
    const int64_t LD = (int64_t)L * D;
    const float* modd = w.tprojd;  // (the tangent of table + tproj is tproj's)
    int rc;
    HIP_TRY(launch_wan_mod(h->P(b.sst), w.tproj, w.mod, BF, 6, D, s));
    // 1. self-attention over the whole video
    HIP_TRY(launch_wan_ln_modulate_jvp(D, w.x[0], w.xd[0], w.mod, modd, 6 * D, 0, D, w.y, w.yd, M, fs, 1e-6f, s));
    if ((rc = wan_gemm(WanOperand{w.y}, b.p_qkv, b.b_qkv, w.qkv, M, 3 * D, D, s)) ||
        (rc = wan_gemm(WanOperand{w.yd}, b.p_qkv, nullptr, w.qkvd, M, 3 * D, D, s)))
        return rc;
    const __bf16 *qkv = (const __bf16*)w.qkv, *qkvd = (const __bf16*)w.qkvd;
    HIP_TRY(launch_wan_rms_rope_jvp(D, qkv, qkvd, 3 * D, h->P(b.nq), c.eps, w.cs, w.qn, w.qnd, LD, D, M, L, s));
    HIP_TRY(launch_wan_rms_rope_jvp(D, qkv + D, qkvd + D, 3 * D, h->P(b.nk), c.eps, w.cs, w.kf, w.kfd, LD, D, M, L, s));
    HIP_TRY(launch_rms_rope(D, qkv + 2 * D, 3 * D, nullptr, c.eps, nullptr, w.vf, LD, 0, D, M, L, s));
    HIP_TRY(launch_rms_rope(D, qkvd + 2 * D, 3 * D, nullptr, c.eps, nullptr, w.vfd, LD, 0, D, M, L, s));
    HIP_TRY(launch_wan_attention_jvp(w.qn, w.qnd, D, LD, w.kf, w.vf, w.kfd, w.vfd, D, LD, w.att, w.attd, D, LD, batch, h->H, L, L, s));
    if ((rc = wan_jvp_residual(w, w.att, w.attd, b.p_o, h->P(b.o_b), w.mod + 2 * D, modd + 2 * D, 6 * D, fs, M, D, D, s))) return rc;
    // 2. cross-attention to the text: a constant affine in front, keys and values without a tangent, no gate behind
    HIP_TRY(launch_wan_ln_modulate_jvp(D, w.x[0], w.xd[0], b.n2mod, nullptr, 0, 0, D, w.y, w.yd, M, M, 1e-6f, s));
    if ((rc = wan_gemm(WanOperand{w.y}, b.p_q2, h->P(b.q2_b), w.qkv, M, D, D, s, 0, nullptr, 0, 1, nullptr, w.gs, w.gs_bytes)) ||
        (rc = wan_gemm(WanOperand{w.yd}, b.p_q2, nullptr, w.qkvd, M, D, D, s, 0, nullptr, 0, 1, nullptr, w.gs, w.gs_bytes)))
        return rc;
    HIP_TRY(launch_wan_rms_rope_jvp(D, w.qkv, w.qkvd, D, h->P(b.nq2), c.eps, nullptr, w.qn, w.qnd, LD, D, M, L, s));
    HIP_TRY(launch_wan_attention_jvp(w.qn, w.qnd, D, LD, b.kv2, (const __bf16*)b.kv2 + D, nullptr, nullptr, 2 * D, (int64_t)h->cur.text_L * 2 * D, w.att,
                                     w.attd, D, LD, batch, h->H, L, h->cur.text_L, s));
    if ((rc = wan_jvp_residual(w, w.att, w.attd, b.p_o2, h->P(b.o2_b), nullptr, nullptr, 0, 1, M, D, D, s))) return rc;
    // 3. feed-forward: the pre-activation is stored (bf16, the token GEMM's output type) and the GELU is a pass of its own
    HIP_TRY(launch_wan_ln_modulate_jvp(D, w.x[0], w.xd[0], w.mod, modd, 6 * D, 3 * D, 4 * D, w.y, w.yd, M, fs, 1e-6f, s));
    if ((rc = wan_gemm(WanOperand{w.y}, b.p_f0, h->P(b.f0_b), w.hid, M, h->Fd, D, s)) ||
        (rc = wan_gemm(WanOperand{w.yd}, b.p_f0, nullptr, w.hidd, M, h->Fd, D, s)))
        return rc;
    HIP_TRY(launch_wan_gelu_jvp(w.hid, w.hidd, w.hid, w.hidd, (int64_t)M * h->Fd, s));
    return wan_jvp_residual(w, w.hid, w.hidd, b.p_f2, h->P(b.f2_b), w.mod + 5 * D, modd + 5 * D, 6 * D, fs, M, D, h->Fd, s);
}

bool wan_jvp_shape_ok(int batch, int frames, int height, int width) {
    return wan_shape_ok(batch, frames, height, width) && wan_rows_fit(batch, frames, height, width);
}

}  // namespace

extern "C" {

size_t fg_wan_jvp_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width) {
    if (!h || h->fp8 || wan_variant(h) || !wan_jvp_shape_ok(batch, frames, height, width)) return 0;
    Arena A;
    A.dry = true;
    WanJvpWs w;
    return wan_jvp_plan(h, batch, frames, height / 2, width / 2, A, w);
}

int fg_wan_jvp(fg_wan* h, const float* x_t, const float* t_frames, const float* r_frames, const float* v_x, const float* vt_frames,
               const float* vr_frames, float* out, float* jvp, int batch, int frames, int height, int width, const int* skip_layers, int num_skip,
               void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !x_t || !t_frames || !v_x || !out || !jvp) return fail(FG_EINVAL, "fg_wan_jvp: null argument");
    int rc;
    if ((rc = wan_jvp_refusal(h))) return rc;
    if (skip_layers || num_skip != 0) return fail(FG_EINVAL, "fg_wan_jvp: skip_layers is not implemented");
    if (r_frames && !h->ext.r_timestep) return fail(FG_EINVAL, "fg_wan_jvp: r_frames given, but the handle has no r_embedder (fg_wan_create_ex, r_timestep = 1)");
    if (vr_frames && !r_frames) return fail(FG_EINVAL, "fg_wan_jvp: vr_frames given without r_frames");
    if (!wan_jvp_shape_ok(batch, frames, height, width) || !workspace || (((uintptr_t)workspace) & 255))
        return fail(FG_EINVAL, "fg_wan_jvp: bad batch / frames / size / workspace");
    if (out == x_t || out == v_x) return fail(FG_EINVAL, "fg_wan_jvp: out must not alias x_t or v_x");
    if (jvp == out || jvp == x_t || jvp == v_x || (const float*)jvp == t_frames || (const float*)jvp == r_frames || (const float*)jvp == vt_frames ||
        (const float*)jvp == vr_frames)
        return fail(FG_EINVAL, "fg_wan_jvp: jvp must not alias another argument");
    const fg_wan_config& c = h->cfg;
    if (frames > c.rope_max_seq_len) return fail(FG_EINVAL, "fg_wan_jvp: %d frames exceed the RoPE table (rope_max_seq_len = %d)", frames, c.rope_max_seq_len);
    const int D = h->D, gh = height / 2, gw = width / 2, fs = gh * gw, BF = batch * frames, L = frames * fs, M = batch * L;
    if (gh > c.rope_max_seq_len || gw > c.rope_max_seq_len) return fail(FG_EINVAL, "fg_wan_jvp: grid exceeds the RoPE table");
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_wan_pack_weights)");
    if ((rc = wan_conditions_ready(h, batch, frames, height, width))) return rc;
    Arena A;
    A.base = (char*)workspace;
    WanJvpWs w;
    const size_t need = wan_jvp_plan(h, batch, frames, gh, gw, A, w);
    if (need > workspace_bytes) return fail(FG_ENOMEM, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    // the zero rows: a null vt / vr, and the bias of the tangent's patch embedding (zrow | zbias are neighbours in the plan)
    HIP_TRY(hipMemsetAsync(w.zrow, 0, (size_t)((char*)w.rrow - (char*)w.zrow), s));
    const float* vt = vt_frames ? vt_frames : w.zrow;
    // 1. time conditioning
    if ((rc = wan_jvp_embedder(h, t_frames, vt, h->t1_w, h->t1_b, h->t2_w, h->t2_b, h->tp_w, h->tp_b, w.temb, w.tembd, w.tproj, w.tprojd, BF, w, s)))
        return rc;
    if (r_frames) {
        // the r_embedder sees r, or t - r for time_cond_type "diff"; its tangent rows are formed the same way from vt and vr
        const float* vr = vr_frames ? vr_frames : w.zrow;
        HIP_TRY(launch_wan_r_rows(t_frames, r_frames, h->ext.time_cond_diff, w.rrow, BF, s));
        HIP_TRY(launch_wan_r_rows(vt, vr, h->ext.time_cond_diff, w.rrowd, BF, s));
        if ((rc = wan_jvp_embedder(h, w.rrow, w.rrowd, h->r1_w, h->r1_b, h->r2_w, h->r2_b, h->rp_w, h->rp_b, w.e, w.ed, w.rproj, w.rprojd, BF, w, s)))
            return rc;
        HIP_TRY(launch_wan_add_r(w.temb, w.e, (int64_t)BF * D, w.tproj, w.rproj, (int64_t)BF * 6 * D, s));
        HIP_TRY(launch_wan_add_r(w.tembd, w.ed, (int64_t)BF * D, w.tprojd, w.rprojd, (int64_t)BF * 6 * D, s));
    }
    HIP_TRY(launch_wan_rope_table(h->tab_t, h->tab_h, h->tab_w, w.cs, L, fs, gw, 0, c.rope_max_seq_len, h->npt, h->nph, h->npw, s));
    // 2. patch embedding (linear: the tangent is the embedding of v_x without the bias)
    const WanEmbedSrc src{x_t, nullptr, WAN_EMBED_PLAIN, c.in_channels, frames, height, width};
    const WanEmbedSrc srcd{v_x, nullptr, WAN_EMBED_PLAIN, c.in_channels, frames, height, width};
    HIP_TRY(launch_wan_embed(src, h->P(h->pe_w), h->P(h->pe_b), w.x[0], batch, D, L, 0, s));
    HIP_TRY(launch_wan_embed(srcd, h->P(h->pe_w), w.zbias, w.xd[0], batch, D, L, 0, s));
    // 3. blocks
    for (fg_wan::Blk& b : h->blocks)
        if ((rc = wan_jvp_block(h, b, w, batch, fs, L, M, BF, s))) return rc;
    // 4. output layer
    HIP_TRY(launch_wan_outmod(h->P(h->sst), w.temb, w.omod, BF, D, s));
    HIP_TRY(launch_wan_dup2(w.tembd, w.omodd, BF, D, s));
    HIP_TRY(launch_wan_final_jvp(D, w.x[0], w.xd[0], w.omod, w.omodd, h->P(h->po_w), h->P(h->po_b), out, jvp, M, frames, gh, gw, c.out_channels, c.eps,
                                 s));
    return FG_OK;
}

// ---- handle-free entry points of wan_jvp.hip's kernels (the per-op tests and timings) --------------------------------------------
int fg_op_wan_attention_jvp(const void* q, const void* qd, int ldq, int64_t q_bs, const void* k, const void* v, const void* kd, const void* vd, int ldk,
                            int64_t kv_bs, void* out, void* outd, int ldo, int64_t o_bs, int batch, int heads, int lq, int lkv, void* stream) {
    if (!q || !k || !v || !out || !outd || out == outd || ldq <= 0 || ldk <= 0 || ldo <= 0 || (ldq % 8) || (ldk % 8) || (ldo % 4) || q_bs < 0 ||
        kv_bs < 0 || o_bs < 0 || batch <= 0 || heads <= 0 || lq <= 0 || lkv <= 0)
        return fail(FG_EINVAL, "fg_op_wan_attention_jvp: bad argument (null pointer, out == outd, ldq %% 8, ldk %% 8, ldo %% 4, a negative stride or count)");
    // the kernel's 16-byte operand loads and 8-byte stores: every sample's rows start aligned
    if ((q_bs % 8) || (kv_bs % 8) || (o_bs % 4) || (((uintptr_t)q | (uintptr_t)qd | (uintptr_t)k | (uintptr_t)v | (uintptr_t)kd | (uintptr_t)vd) & 15) ||
        (((uintptr_t)out | (uintptr_t)outd) & 7))
        return fail(FG_EINVAL, "fg_op_wan_attention_jvp: q / qd / k / v / kd / vd must be 16-byte aligned with q_bs %% 8 and kv_bs %% 8, out / outd "
                    "8-byte aligned with o_bs %% 4");
    HIP_TRY(launch_wan_attention_jvp(q, qd, ldq, q_bs, k, v, kd, vd, ldk, kv_bs, out, outd, ldo, o_bs, batch, heads, lq, lkv, (hipStream_t)stream));
    return FG_OK;
}

namespace {
bool wan_jvp_width_ok(int d) { return d == 256 || d == 384 || d == 1536 || d == 2048 || d == 3072 || d == 5120; }
}  // namespace

int fg_op_wan_modulate_jvp(const void* x, const void* xd, const float* mod, const float* modd, int mod_stride, int shift_off, int scale_off, void* y,
                           void* yd, int ntok, int d, int tokens_per_row, float eps, void* stream) {
    if (!x || !xd || !mod || !y || !yd || y == yd || ntok <= 0 || tokens_per_row <= 0 || !wan_jvp_width_ok(d) || mod_stride < 0 || (mod_stride % 2) ||
        shift_off < 0 || (shift_off % 2) || scale_off < 0 || (scale_off % 2))
        return fail(FG_EINVAL, "fg_op_wan_modulate_jvp: bad argument (null pointer, y == yd, a count <= 0, d not one of 256, 384, 1536, 2048, 3072, "
                    "5120, an odd or negative stride / offset)");
    HIP_TRY(launch_wan_ln_modulate_jvp(d, x, xd, mod, modd, mod_stride, shift_off, scale_off, y, yd, ntok, tokens_per_row, eps, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_wan_rms_rope_jvp(const void* src, const void* srcd, int ld_src, const float* w, float eps, const float* cs, void* dst, void* dstd, int rows,
                           int l, int d, void* stream) {
    if (!src || !srcd || !w || !dst || !dstd || dst == dstd || rows <= 0 || l <= 0 || (rows % l) || !wan_jvp_width_ok(d) || ld_src < d || (ld_src % 2))
        return fail(FG_EINVAL, "fg_op_wan_rms_rope_jvp: bad argument (null pointer, dst == dstd, rows not a multiple of l, d not one of 256, 384, "
                    "1536, 2048, 3072, 5120, ld_src < d or odd)");
    HIP_TRY(launch_wan_rms_rope_jvp(d, src, srcd, ld_src, w, eps, (const float2*)cs, dst, dstd, (int64_t)l * d, d, rows, l, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_wan_gelu_jvp(const void* h, const void* hd, void* a, void* ad, int64_t n, void* stream) {
    if (!h || !hd || !a || !ad || a == ad || n <= 0 || (n % 4)) return fail(FG_EINVAL, "fg_op_wan_gelu_jvp: bad argument (null pointer, a == ad, n %% 4)");
    HIP_TRY(launch_wan_gelu_jvp(h, hd, a, ad, n, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_wan_final_jvp(const void* tokens, const void* tokens_d, const float* mod, const float* modd, const float* w, const float* bias, float* out,
                        float* outd, int batch, int channels, int frames, int gh, int gw, int d, float eps, void* stream) {
    if (!tokens || !tokens_d || !mod || !modd || !w || !bias || !out || !outd || out == outd || batch <= 0 || channels <= 0 || channels > 64 ||
        frames <= 0 || gh <= 0 || gw <= 0 || !wan_jvp_width_ok(d))
        return fail(FG_EINVAL, "fg_op_wan_final_jvp: bad argument (null pointer, out == outd, channels outside [1, 64], a count <= 0, d not one of "
                    "256, 384, 1536, 2048, 3072, 5120)");
    if ((int64_t)batch * frames * gh * gw > INT32_MAX / 2) return fail(FG_EINVAL, "fg_op_wan_final_jvp: too many tokens");
    HIP_TRY(launch_wan_final_jvp(d, tokens, tokens_d, mod, modd, w, bias, out, outd, batch * frames * gh * gw, frames, gh, gw, channels, eps,
                                 (hipStream_t)stream));
    return FG_OK;
}
