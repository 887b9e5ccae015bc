// EDM2 forward-mode derivative (EDM2Precond.jvp; the sCM tangent of the reference's SCMModel._jvp): fg_edm2_jvp runs the primal forward
// of engine_edm2.inc - the same kernels in the same order, so `out` is fg_edm2_forward's to the bit - and, interleaved block by block,
// the tangent stream on its own buffers (edm2_jvp.hip).  A tangent convolution is the primal's adm_launch_conv on the tangent operand
// with the same packed weights and no prologue.  Textually included by engine.hip behind engine_edm2.inc.
}  // extern "C" (reopened below)

namespace {

struct E2JWs {
    E2Ws p;  // the primal forward's buffers, laid out first exactly as fg_edm2_forward lays them out
    float *ct, *four, *e, *emb, *cc;
    float* stem_in;
    std::vector<float*> skip;
    float *xa, *xb, *op, *h, *s, *t1, *qkv, *a, *F;
};

size_t e2j_plan(const fg_edm2* h, int B, Arena& A, E2JWs& w) {
    e2_plan(h, B, A, w.p);
    const fg_edm2_config& c = h->cfg;
    size_t max_act = 0, max_attn = 1, max_op = 0;
    for (const auto* list : {&h->enc, &h->dec})
        for (const E2Block& b : *list) {
            const size_t hw = (size_t)b.res_out * b.res_out;
            max_act = std::max(max_act, hw * b.cout);
            if (b.attn) max_attn = std::max(max_attn, hw * b.cout);
            // conv_res0's operand at its source resolution (the up block's: res_in), conv_res1's at res_out
            const size_t hw0 = b.up ? (size_t)b.res_in * b.res_in : hw;
            max_op = std::max(max_op, std::max(hw0 * (b.enc ? b.cout : b.cin), hw * b.cout));
        }
    const int R = c.img_resolution;
    w.ct = A.get<float>(8 * (size_t)B);
    w.four = A.get<float>((size_t)B * h->cnoise);
    w.e = A.get<float>((size_t)B * h->cemb);
    w.emb = A.get<float>((size_t)B * h->cemb);
    w.cc = A.get<float>((size_t)B * h->total);
    w.stem_in = A.get<float>((size_t)B * R * R * kE2StemPad);
    w.skip.clear();
    for (size_t i = 0; i < h->skip_c.size(); ++i) w.skip.push_back(A.get<float>((size_t)B * h->skip_res[i] * h->skip_res[i] * h->skip_c[i]));
    w.xa = A.get<float>((size_t)B * max_act);
    w.xb = A.get<float>((size_t)B * max_act);
    w.op = A.get<float>((size_t)B * max_op);
    w.h = A.get<float>((size_t)B * max_act);
    w.s = A.get<float>((size_t)B * max_act);
    w.t1 = A.get<float>((size_t)B * max_attn);
    w.qkv = A.get<float>((size_t)B * 3 * max_attn);
    w.a = A.get<float>((size_t)B * max_attn);
    w.F = A.get<float>((size_t)B * c.img_channels * R * R);
    return (A.off + 255) & ~(size_t)255;
}

// tangent of e2_modulation: c_d = emb_linear(emb_d, gain = emb_gain) for every block
int e2j_modulation(fg_edm2* h, const float* emb_d, int B, E2JWs& w, hipStream_t s) {
    HIP_TRY(launch_linear(emb_d, h->w_mod, nullptr, w.cc, B, h->cemb, h->total, 0, s));
    return FG_OK;
}

// e2_block with the tangent of every step behind (or, where it reads a buffer the primal step overwrites, in front of) that step.
// x1_d / x2_d: tangents of x1 / x2; dst_d: the tangent of dst.  The primal launches are e2_block's, argument for argument.
int e2j_block(fg_edm2* h, const E2Block& b, const float* x1, const float* x1_d, int c1, const float* x2, const float* x2_d, int c2, float* dst,
              float* dst_d, int B, E2JWs& w, hipStream_t s) {
    const fg_edm2_config& c = h->cfg;
    E2Ws& p = w.p;
    const int Ho = b.res_out;
    const int64_t hw = (int64_t)Ho * Ho;
    const float clip = c.clip_act > 0 ? (float)c.clip_act : 0.f;
    const float res_skip = (float)((1 - c.res_balance) / mp_sum_norm(c.res_balance));
    const float attn_skip = (float)((1 - c.attn_balance) / mp_sum_norm(c.attn_balance));
    AdmConvArgs r0;
    r0.Hs = r0.H = Ho, r0.B = B, r0.silu = 1, r0.ab = h->ones, r0.ab_stride = 0;
    const float *resid = nullptr, *resid_d = nullptr, *src1_d = x1_d, *src2_d = nullptr;
    int resid_mode = 0;
    if (b.enc) {
        if (b.skip >= 0) {
            AdmConvArgs k;
            k.src1 = x1, k.C1 = c1, k.Hs = k.H = Ho, k.B = B, k.w = b.p_skip, k.out = p.s, k.Cout = b.cout;
            HIP_TRY(adm_launch_conv(h->cmode, 1, k, s));
            k.src1 = x1_d, k.out = w.s;
            HIP_TRY(adm_launch_conv(h->cmode, 1, k, s));
            HIP_TRY(edm2_launch_pixel_norm_jvp(p.s, w.s, w.s, B, Ho, b.cout, 0, s));  // reads the conv's output before its norm
            HIP_TRY(edm2_launch_pixel_norm(p.s, p.s, B, Ho, b.cout, 0, s));
        } else {
            HIP_TRY(edm2_launch_pixel_norm(x1, p.s, B, Ho, b.cout, b.down ? 1 : 0, s));
            HIP_TRY(edm2_launch_pixel_norm_jvp(x1, x1_d, w.s, B, Ho, b.cout, b.down ? 1 : 0, s));
        }
        r0.src1 = p.s, r0.C1 = b.cout;
        resid = p.s, resid_d = w.s, src1_d = w.s;
    } else if (b.up) {
        r0.src1 = x1, r0.C1 = c1, r0.Hs = b.res_in, r0.res_mode = 2;
        resid = x1, resid_d = x1_d, resid_mode = 2;
    } else if (c2) {
        r0.src1 = x1, r0.src2 = x2, r0.C1 = c1, r0.C2 = c2, r0.ab = b.cat_ab;
        src2_d = x2_d;
        AdmConvArgs k;
        k.src1 = x1, k.src2 = x2, k.C1 = c1, k.C2 = c2, k.Hs = k.H = Ho, k.B = B, k.w = b.p_skip, k.out = p.s, k.Cout = b.cout;
        HIP_TRY(adm_launch_conv(h->cmode, 1, k, s));
        k.src1 = x1_d, k.src2 = x2_d, k.out = w.s;
        HIP_TRY(adm_launch_conv(h->cmode, 1, k, s));
        resid = p.s, resid_d = w.s;
    } else {
        r0.src1 = x1, r0.C1 = c1;
        resid = x1, resid_d = x1_d;
    }
    r0.w = b.p_res0, r0.out = p.h, r0.Cout = b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 3, r0, s));
    // conv_res0's tangent: the operand silu'(a x) a x_d at the source resolution, then the same conv without a prologue
    HIP_TRY(edm2_launch_silu_operand_jvp(r0.src1, r0.src2, src1_d, src2_d, r0.C1, r0.C2, r0.ab, 0, nullptr, 0, w.op, B, (int64_t)r0.Hs * r0.Hs, s));
    AdmConvArgs t0;
    t0.src1 = w.op, t0.C1 = r0.C1 + r0.C2, t0.Hs = r0.Hs, t0.H = Ho, t0.B = B, t0.res_mode = r0.res_mode, t0.w = b.p_res0, t0.out = w.h,
    t0.Cout = b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 3, t0, s));
    AdmConvArgs r1;
    r1.src1 = p.h, r1.C1 = b.cout, r1.Hs = r1.H = Ho, r1.B = B;
    r1.ab = p.ab_all + b.off, r1.ab_stride = h->total, r1.silu = 1, r1.w = b.p_res1;
    r1.resid = resid, r1.resid_mode = resid_mode, r1.resid_scale = res_skip;
    r1.clip = b.attn ? 0.f : clip, r1.out = b.attn ? p.t1 : dst, r1.Cout = b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 3, r1, s));
    // conv_res1's tangent: silu'(c h) (c h_d + c_d h), the residual's tangent with the same weight, no clamp
    HIP_TRY(edm2_launch_silu_operand_jvp(p.h, nullptr, w.h, nullptr, b.cout, 0, r1.ab, h->total, w.cc + b.off, h->total, w.op, B, hw, s));
    AdmConvArgs t1;
    t1.src1 = w.op, t1.C1 = b.cout, t1.Hs = t1.H = Ho, t1.B = B, t1.w = b.p_res1;
    t1.resid = resid_d, t1.resid_mode = resid_mode, t1.resid_scale = res_skip;
    t1.out = b.attn ? w.t1 : dst_d, t1.Cout = b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 3, t1, s));
    if (!b.attn) {
        if (clip > 0.f) HIP_TRY(edm2_launch_clamp_jvp(dst, dst_d, clip, (int64_t)B * hw * b.cout, s));
        return FG_OK;
    }
    AdmConvArgs q;
    q.src1 = p.t1, q.C1 = b.cout, q.Hs = q.H = Ho, q.B = B, q.w = b.p_qkv, q.out = p.qkv, q.Cout = 3 * b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 1, q, s));
    q.src1 = w.t1, q.out = w.qkv;
    HIP_TRY(adm_launch_conv(h->cmode, 1, q, s));
    HIP_TRY(adm_launch_attention_mp(p.qkv, p.a, B, Ho * Ho, b.cout / 64, s));
    HIP_TRY(edm2_launch_attention_mp_jvp(p.qkv, w.qkv, nullptr, w.a, B, Ho * Ho, b.cout / 64, s));
    AdmConvArgs pr;
    pr.src1 = p.a, pr.C1 = b.cout, pr.Hs = pr.H = Ho, pr.B = B, pr.w = b.p_proj;
    pr.resid = p.t1, pr.resid_scale = attn_skip, pr.clip = clip, pr.out = dst, pr.Cout = b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 1, pr, s));
    pr.src1 = w.a, pr.resid = w.t1, pr.clip = 0.f, pr.out = dst_d;
    HIP_TRY(adm_launch_conv(h->cmode, 1, pr, s));
    if (clip > 0.f) HIP_TRY(edm2_launch_clamp_jvp(dst, dst_d, clip, (int64_t)B * hw * b.cout, s));
    return FG_OK;
}

// e2_forward with the tangent along (vx, vt) interleaved; vt nullable (= 0)
int e2j_forward(fg_edm2* h, const float* x_t, const double* t, const float* labels, const float* vx, const float* vt, float* out, float* jvp,
                int B, E2JWs& w, hipStream_t s) {
    const fg_edm2_config& c = h->cfg;
    E2Ws& p = w.p;
    HIP_TRY(launch_precond_coef(t, 1, nullptr, 0, c.sigma_data, h->shift(), 1e-6, c.drop_precond, p.coef, B, s));
    // ct: c_in, c_in_d, c_noise_d, -, c_skip, c_skip_d, c_out, c_out_d
    HIP_TRY(launch_jvp_coef(t, nullptr, vt, nullptr, c.sigma_data, h->shift(), c.drop_precond, w.ct, B, s));
    const float *c_in_d = w.ct + B, *c_noise_d = w.ct + 2 * (size_t)B, *c_skip_d = w.ct + 5 * (size_t)B, *c_out_d = w.ct + 7 * (size_t)B;
    HIP_TRY(edm2_launch_fourier(p.coef + B, h->P(h->freqs), h->P(h->phases), p.four, B, h->cnoise, s));
    HIP_TRY(edm2_launch_fourier_jvp(p.coef + B, c_noise_d, h->P(h->freqs), h->P(h->phases), w.four, B, h->cnoise, s));
    HIP_TRY(launch_linear(p.four, h->w_noise, nullptr, p.e, B, h->cnoise, h->cemb, 0, s));
    HIP_TRY(launch_linear(w.four, h->w_noise, nullptr, w.e, B, h->cnoise, h->cemb, 0, s));
    const bool lab = c.label_dim && labels;
    if (lab) HIP_TRY(launch_linear(labels, h->w_label, nullptr, p.lab, B, c.label_dim, h->cemb, 0, s));
    HIP_TRY(edm2_launch_emb_finish(p.e, lab ? p.lab : nullptr, p.emb, (int64_t)B * h->cemb, s));
    HIP_TRY(edm2_launch_emb_finish_jvp(p.e, lab ? p.lab : nullptr, w.e, w.emb, (int64_t)B * h->cemb, s));
    int rc;
    if ((rc = e2_modulation(h, p.emb, B, p, s)) || (rc = e2j_modulation(h, w.emb, B, w, s))) return rc;
    const int R = c.img_resolution;
    HIP_TRY(edm2_launch_stem_operand(x_t, p.coef, p.stem_in, B, c.img_channels, R, kE2StemPad, s));
    HIP_TRY(edm2_launch_stem_operand_jvp(x_t, vx, p.coef, c_in_d, w.stem_in, B, c.img_channels, R, kE2StemPad, s));
    AdmConvArgs st;
    st.src1 = p.stem_in, st.C1 = kE2StemPad, st.Hs = st.H = R, st.B = B, st.w = h->p_stem, st.out = p.skip[0], st.Cout = h->stem_c;
    HIP_TRY(adm_launch_conv(h->cmode, 3, st, s));
    st.src1 = w.stem_in, st.out = w.skip[0];
    HIP_TRY(adm_launch_conv(h->cmode, 3, st, s));
    const float *x = p.skip[0], *x_d = w.skip[0];
    int xc = h->stem_c;
    for (size_t i = 0; i < h->enc.size(); ++i) {
        const E2Block& b = h->enc[i];
        if ((rc = e2j_block(h, b, x, x_d, xc, nullptr, nullptr, 0, p.skip[i + 1], w.skip[i + 1], B, w, s))) return rc;
        x = p.skip[i + 1], x_d = w.skip[i + 1], xc = b.cout;
    }
    int sp = (int)p.skip.size();
    float *pong[2] = {p.xa, p.xb}, *pong_d[2] = {w.xa, w.xb};
    int cur = 0;
    for (const E2Block& b : h->dec) {
        if (b.skip_c) --sp;
        const float *x2 = b.skip_c ? p.skip[sp] : nullptr, *x2_d = b.skip_c ? w.skip[sp] : nullptr;
        if ((rc = e2j_block(h, b, x, x_d, xc, x2, x2_d, b.skip_c, pong[cur], pong_d[cur], B, w, s))) return rc;
        x = pong[cur], x_d = pong_d[cur], xc = b.cout;
        cur ^= 1;
    }
    AdmConvArgs o;
    o.src1 = x, o.C1 = h->out_cin, o.Hs = o.H = R, o.B = B, o.w = h->p_out, o.out = p.F, o.Cout = c.img_channels;
    HIP_TRY(adm_launch_conv(h->cmode, 3, o, s));
    o.src1 = x_d, o.out = w.F;
    HIP_TRY(adm_launch_conv(h->cmode, 3, o, s));
    HIP_TRY(edm2_launch_precond_out(p.F, x_t, p.coef + 2 * (size_t)B, p.coef + 3 * (size_t)B, out, B, c.img_channels, R, s));
    HIP_TRY(edm2_launch_precond_out_jvp(p.F, w.F, x_t, vx, p.coef + 2 * (size_t)B, c_skip_d, p.coef + 3 * (size_t)B, c_out_d, jvp, B,
                                        c.img_channels, R, s));
    return FG_OK;
}

// the jvp entry points size their own check: a short workspace is an argument error here (FG_EINVAL), found before any launch
int e2j_setup(const fg_edm2* h, int B, void* workspace, size_t bytes, E2JWs& w) {
    if (B <= 0) return fail(FG_EINVAL, "batch must be positive");
    if (!workspace) return fail(FG_EINVAL, "workspace is null");
    if (((uintptr_t)workspace) & 255) return fail(FG_EINVAL, "workspace must be 256-byte aligned");
    Arena A;
    A.base = (char*)workspace;
    const size_t need = e2j_plan(h, B, A, w);
    if (need > bytes) return fail(FG_EINVAL, "workspace too small: need %zu bytes for batch %d (fg_edm2_jvp_workspace_bytes), got %zu", need, B, bytes);
    return FG_OK;
}

}  // namespace

extern "C" {

size_t fg_edm2_jvp_workspace_bytes(const fg_edm2* h, int batch) {
    if (!h || batch <= 0) return 0;
    Arena A;
    A.dry = true;
    E2JWs w;
    return e2j_plan(h, batch, A, w);
}

int fg_edm2_jvp(fg_edm2* h, const float* x_t, const double* t, const float* class_labels, const float* vx, const float* vt, float* out,
                float* jvp, int batch, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !x_t || !t || !vx || !out || !jvp) return fail(FG_EINVAL, "null argument");
    if (out == x_t || jvp == x_t || out == vx || jvp == vx || out == jvp) return fail(FG_EINVAL, "out and jvp must not alias x_t, vx or each other");
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_edm2_pack_weights)");
    E2JWs w;
    const int rc = e2j_setup(h, batch, workspace, workspace_bytes, w);
    if (rc) return rc;
    return e2j_forward(h, x_t, t, class_labels, vx, vt, out, jvp, batch, w, (hipStream_t)stream);
}

int fg_edm2_run_block_jvp(fg_edm2* h, int index, const float* x1, const float* x1_d, int c1, const float* x2, const float* x2_d, int c2,
                          const float* emb, const float* emb_d, float* out, float* out_d, int batch, void* workspace, size_t workspace_bytes,
                          void* stream) {
    if (!h || !x1 || !x1_d || !emb || !emb_d || !out || !out_d) return fail(FG_EINVAL, "null argument");
    const E2Block* b = e2_block_at(h, index);
    if (!b) return fail(FG_EINVAL, "block index out of range");
    if (c1 <= 0 || c2 != b->skip_c || c1 + c2 != b->cin)
        return fail(FG_EINVAL, "%s: channel split c1 = %d, c2 = %d; the block takes %d + %d (its skip)", b->key.c_str(), c1, c2,
                    b->cin - b->skip_c, b->skip_c);
    if (c2 && (!x2 || !x2_d)) return fail(FG_EINVAL, "%s: x2 or x2_d is null", b->key.c_str());
    if (out == out_d) return fail(FG_EINVAL, "out_d must not alias out");
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_edm2_pack_weights)");
    E2JWs w;
    int rc = e2j_setup(h, batch, workspace, workspace_bytes, w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = e2_modulation(h, emb, batch, w.p, s)) || (rc = e2j_modulation(h, emb_d, batch, w, s))) return rc;
    return e2j_block(h, *b, x1, x1_d, c1, c2 ? x2 : nullptr, c2 ? x2_d : nullptr, c2, out, out_d, batch, w, s);
}

int fg_op_edm2_attention_jvp(const float* qkv, const float* qkv_d, float* out, float* out_d, int batch, int t, int heads, void* stream) {
    if (t <= 0 || t % 64 || heads <= 0 || heads > 65535 || batch <= 0 || batch > 65535)
        return fail(FG_EINVAL, "fg_op_edm2_attention_jvp: t %d (a positive multiple of 64), heads %d, batch %d (1 .. 65535)", t, heads, batch);
    if (!qkv || !qkv_d || !out_d || out == out_d) return fail(FG_EINVAL, "fg_op_edm2_attention_jvp: null pointer, or out aliases out_d");
    HIP_TRY(edm2_launch_attention_mp_jvp(qkv, qkv_d, out, out_d, batch, t, heads, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_edm2_pixel_norm_jvp(const float* x, const float* x_d, float* out_d, int batch, int h, int c, int down, void* stream) {
    if (batch <= 0 || batch > 65535 || h <= 0 || h > 4096 || c <= 0 || c > (1 << 16) || (down != 0 && down != 1))
        return fail(FG_EINVAL, "fg_op_edm2_pixel_norm_jvp: batch %d (1 .. 65535), h %d (1 .. 4096), c %d (1 .. 65536), down %d (0, 1)", batch, h,
                    c, down);
    if ((int64_t)batch * h * h > ((int64_t)1 << 31)) return fail(FG_EINVAL, "fg_op_edm2_pixel_norm_jvp: more than 2^31 pixels");
    if (!x || !x_d || !out_d || out_d == x) return fail(FG_EINVAL, "fg_op_edm2_pixel_norm_jvp: null pointer, or out_d aliases x");
    if (down && out_d == x_d) return fail(FG_EINVAL, "fg_op_edm2_pixel_norm_jvp: in place (out_d == x_d) only with down == 0");
    HIP_TRY(edm2_launch_pixel_norm_jvp(x, x_d, out_d, batch, h, c, down, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_edm2_silu_operand_jvp(const float* x1, const float* x2, const float* d1, const float* d2, int c1, int c2, const float* ab,
                                int ab_stride, const float* ad, int ad_stride, float* out, int batch, int hw, void* stream) {
    if (c1 <= 0 || c1 % 4 || c2 < 0 || c2 % 4 || batch <= 0 || batch > 65535 || hw <= 0 || hw > (1 << 24) || ab_stride < 0 ||
        (ab_stride && ab_stride < c1 + c2) || (ad && ad_stride < c1 + c2))
        return fail(FG_EINVAL, "fg_op_edm2_silu_operand_jvp: c1 %d > 0 and c2 %d >= 0 multiples of 4, batch %d (1 .. 65535), hw %d (1 .. 2^24), "
                    "ab_stride %d (0 or >= c1 + c2), ad_stride %d (>= c1 + c2 with ad)", c1, c2, batch, hw, ab_stride, ad_stride);
    if (!x1 || !d1 || (c2 && (!x2 || !d2)) || !ab || !out) return fail(FG_EINVAL, "fg_op_edm2_silu_operand_jvp: null pointer");
    if (((uintptr_t)x1 | (uintptr_t)d1 | (uintptr_t)(c2 ? x2 : nullptr) | (uintptr_t)(c2 ? d2 : nullptr) | (uintptr_t)out) & 15)
        return fail(FG_EINVAL, "fg_op_edm2_silu_operand_jvp: x1 / x2 / d1 / d2 / out must be 16-byte aligned");
    if (((uintptr_t)ab & 7) || ((uintptr_t)ad & 3)) return fail(FG_EINVAL, "fg_op_edm2_silu_operand_jvp: ab must be 8-byte aligned, ad 4-byte aligned");
    HIP_TRY(edm2_launch_silu_operand_jvp(x1, c2 ? x2 : nullptr, d1, c2 ? d2 : nullptr, c1, c2, (const float2*)ab, ab_stride, ad, ad_stride, out,
                                         batch, hw, (hipStream_t)stream));
    return FG_OK;
}
