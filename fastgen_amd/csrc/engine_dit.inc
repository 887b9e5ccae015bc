// DiT engine (SURVEY §8(f)2): parameter plan with the reference's state-dict names, packed GEMM weights, workspace plan, forward
// orchestration and the C ABI of include/fastgen_amd.h (fg_dit_*).  Textually included by engine.hip inside its `extern "C"` region
// (the handle is a HandleBase; pack_group is engine.hip's).  Reference: fastgen/networks/DiT/network.py:153-201 (DiTBlock),
// :204-225 (OutputProjection), :464-574 (DiT.forward); kernels: dit.hip + conv.hip's token GEMM modes.
}  // extern "C" (reopened below: the structures and helpers are C++)

struct fg_dit : HandleBase {
    fg_dit_config cfg;
    int dtype = 0, cmode = 0;  // as fg_edm: storage of the token tensors (0 fp32 / 1 bf16), arithmetic of the GEMMs (FG_DTYPE_*)
    int D = 0, Hd = 0, hd = 0, T = 0, grid = 0;  // hidden size, MLP hidden size, head dim, tokens per image, patches per side
    struct Blk {
        int qkv_w, qkv_b, proj_w, proj_b, fc1_w, fc1_b, fc2_w, fc2_b, mod_w, mod_b;
        void *p_qkv = nullptr, *p_proj = nullptr, *p_fc1 = nullptr, *p_fc2 = nullptr;  // packed (owned)
    };
    std::vector<Blk> blocks;
    int pos = -1, xw = -1, xb = -1, tw0 = -1, tb0 = -1, tw2 = -1, tb2 = -1, rw0 = -1, rb0 = -1, rw2 = -1, rb2 = -1, ytab = -1, fw = -1, fb = -1,
        fmw = -1, fmb = -1;
    void* p_modw = nullptr;   // bf16 GEMM path: all blocks' conditioning_net weights stacked [depth * 6 D][D] bf16 ...
    float* modb = nullptr;    // ... and their biases [depth * 6 D]: one GEMM per forward instead of one 256-row linear per block
    SamplerCache sampler;  // fg_dit_sampler_run (engine_sampler.inc)
    bool gemm3 = false;  // bf16x3 mode: the four block linears on gemm.hip's split-bf16 flavour ([hi | lo | hi] weights, [hi | lo] activation planes)
    // fp8 mode (FG_DTYPE_FP8): cmode / dtype / gemm as in the bf16 mode (token tensors, attention, modulation GEMM, final layer), but the
    // four block linears contract e4m3 operands: p_qkv ... hold [N][K] e4m3fn bytes followed by the N fp32 channel scales
    bool fp8 = false;
    bool gemm = false;  // bf16 mode: the four block linears on gemm.hip (plain [N][K] bf16 weights) instead of conv.hip's token modes
    // a kernel that met an out-of-range class index raises *err_host (pinned, mapped: err_dev is its device address); the next call on
    // the handle reports it (the reference's nn.Embedding device-asserts; nothing is clamped, the sample's output is NaN)
    int *err_host = nullptr, *err_dev = nullptr;
    int take_error() {
        if (!err_host || !*err_host) return 0;
        *err_host = 0;
        return 1;
    }
    // Parameters as the kernels read them.  The four block linears are read from the caller's tensors at PACK time only (into the
    // GEMM layouts of p_qkv ...); every other parameter is copied into `own` at pack time, so that between two packs nothing points into
    // the caller's memory: FSDP2 gathers a group's parameters, packs that group and frees them again (DiT.fully_shard), and a captured
    // sampler graph never holds a pointer to a tensor the caller may reallocate.
    std::vector<float*> own;       // [params]: engine-owned fp32 copy, or nullptr (pack-only parameters, logvar_linear)
    std::vector<char> pack_only;   // [params]
    std::vector<char> dirty;       // [params]: bound since its last pack (or never packed)
    const float* P(int idx) const { return idx < 0 ? nullptr : (own[idx] ? own[idx] : params[idx].ptr); }
    bool is_logvar(int idx) const { return params[idx].name.rfind("logvar_linear", 0) == 0; }
};

namespace {

struct DitWs {
    float *tf, *th, *temb, *remb, *c, *sc, *mod, *fmod, *mod_all;
    void* scb;
    void *x0, *x1, *y, *q, *k, *vt, *att, *hid, *qkv;
    void *y8, *hid8;   // fp8 mode: the quantised A operands [ntok][D] / [ntok][Hd] ...
    float *ys, *hs;    // ... and their per-token scales
};

size_t dit_plan(const fg_dit* h, int B, Arena& A, DitWs& w) {
    const size_t tsz = h->dtype ? 2 : 4;
    const size_t D = h->D, ntok = (size_t)B * h->T;
    w.tf = A.get<float>((size_t)B * 256);
    w.th = A.get<float>((size_t)B * D);
    w.temb = A.get<float>((size_t)B * D);
    w.remb = A.get<float>((size_t)B * D);
    w.c = A.get<float>((size_t)B * D);
    w.sc = A.get<float>((size_t)B * D);
    w.mod = A.get<float>((size_t)B * 6 * D);
    w.mod_all = A.get<float>(h->p_modw && B >= 256 ? (size_t)B * h->blocks.size() * 6 * D : 0);
    w.scb = A.take(h->p_modw && B >= 256 ? (size_t)B * D * 2 : 0);
    w.fmod = A.get<float>((size_t)B * 2 * D);
    w.x0 = A.take(ntok * D * tsz);
    w.x1 = A.take(ntok * D * tsz);
    w.y = A.take(ntok * D * tsz);
    w.q = A.take(2 * (ntok * D + 32 * (size_t)h->T) * (tsz / 2));
    w.k = A.take(2 * (ntok * D + 32 * (size_t)h->T) * (tsz / 2));
    // + 32 rows of slack behind the last head (dit.hip: output tiles past head_dim); in the bf16x3 mode q / k / vt are each two
    // bf16 planes (hi, lo) of ntok * D (+ slack) elements: the same bytes as one fp32 tensor
    w.vt = A.take(2 * (ntok * D + 32 * (size_t)h->T) * (tsz / 2));
    w.att = A.take(ntok * D * tsz);
    w.hid = A.take(ntok * (size_t)h->Hd * tsz);
    w.qkv = A.take(ntok * 3 * D * tsz);  // token-major q | k | v of the LDS-staged attention (bf16 GEMM path, head dim 72)
    w.y8 = A.take(h->fp8 ? ntok * D : 0);
    w.hid8 = A.take(h->fp8 ? ntok * (size_t)h->Hd : 0);
    w.ys = A.get<float>(h->fp8 ? ntok : 0);
    w.hs = A.get<float>(h->fp8 ? ntok : 0);
    return (A.off + 255) & ~(size_t)255;
}

// one token GEMM: out[tok][n] = epilogue(sum_k src[tok][k] W[n][k] + bias[n])
int dit_gemm(fg_dit* h, const void* src, int K, const void* wpack, const float* bias, int N, void* out, int B, hipStream_t s, int act = 0,
             const float* gate = nullptr, int gate_stride = 0, const void* resid = nullptr) {
    if (h->gemm3) {  // src: [hi | lo] planes; out: fp32 (act == 0) or [hi | lo] planes of the GELU'd hidden layer (act == 1)
        GemmArgs g;
        g.A = src; g.W = wpack; g.bias = bias; g.out = out; g.M = B * h->T; g.N = N; g.K = K;
        g.act = act; g.gate = gate; g.gate_stride = gate_stride; g.gate_rows = h->T; g.resid = resid;
        HIP_TRY(launch_gemm_x3(g, act ? 1 : 0, s));
        return FG_OK;
    }
    if (h->gemm) {
        GemmArgs g;
        g.A = src; g.W = wpack; g.bias = bias; g.out = out; g.M = B * h->T; g.N = N; g.K = K;
        g.act = act; g.gate = gate; g.gate_stride = gate_stride; g.gate_rows = h->T; g.resid = resid;
        HIP_TRY(launch_gemm_bf16(g, s));
        return FG_OK;
    }
    ConvArgs a{};
    a.src1 = src; a.C1 = K; a.Hs = a.Ws = a.H = a.W = 16; a.B = B;
    a.wpack = wpack; a.bias = bias; a.scale = 1.0f; a.out = out; a.Cout = N;
    a.act = act; a.gate = gate; a.gate_stride = gate_stride; a.resid = resid;
    HIP_TRY(launch_conv_fused(h->cmode, 1, PRO_NONE, RES_NONE, OUT_TOK, a, s));
    return FG_OK;
}

// the same on e4m3 operands: src [tok][K] bytes + src_scale [tok]; wpack = [N][K] bytes followed by the N channel scales (dit_pack)
int dit_gemm_fp8(fg_dit* h, const void* src, const float* src_scale, int K, const void* wpack, const float* bias, int N, void* out, int B,
                 hipStream_t s, int act = 0, const float* gate = nullptr, int gate_stride = 0, const void* resid = nullptr) {
    GemmArgs g;
    g.A = src; g.W = wpack; g.bias = bias; g.out = out; g.M = B * h->T; g.N = N; g.K = K;
    g.a_scale = src_scale; g.w_scale = reinterpret_cast<const float*>(reinterpret_cast<const char*>(wpack) + (size_t)N * K);
    g.act = act; g.gate = gate; g.gate_stride = gate_stride; g.gate_rows = h->T; g.resid = resid;
    HIP_TRY(launch_gemm_fp8(g, s));
    return FG_OK;
}

// One transformer block in the fp8 mode: LayerNorm-modulate stores e4m3 + scale, the attention output and the GELU'd hidden layer are
// quantised by a pass of their own (their rows cross the producing kernels' tiles); q / k / v, attention and the residual stream stay bf16.
int dit_block_fp8(fg_dit* h, const fg_dit::Blk& b, const float* mod, int mstride, void*& x, void*& xn, int B, DitWs& w, hipStream_t s) {
    const fg_dit_config& c = h->cfg;
    const int D = h->D, T = h->T, ntok = B * T;
    int rc;
    HIP_TRY(launch_dit_ln_modulate_fp8(D, x, mod, mstride, 0, D, w.y8, w.ys, ntok, T, s));
    if (h->hd == 72) {  // qkv stays token-major; attention on wan.hip's LDS-staged kernel
        if ((rc = dit_gemm_fp8(h, w.y8, w.ys, D, b.p_qkv, h->P(b.qkv_b), 3 * D, w.qkv, B, s))) return rc;
        const __bf16* qkv = (const __bf16*)w.qkv;
        HIP_TRY(launch_fa(72, qkv, 3 * D, (int64_t)T * 3 * D, qkv + D, qkv + 2 * D, 3 * D, (int64_t)T * 3 * D, w.att, D, (int64_t)T * D, B,
                          c.num_heads, T, T, s));
    } else {
        GemmArgs g;
        g.A = w.y8; g.W = b.p_qkv; g.bias = h->P(b.qkv_b); g.M = ntok; g.N = 3 * D; g.K = D;
        g.a_scale = w.ys; g.w_scale = reinterpret_cast<const float*>(reinterpret_cast<const char*>(b.p_qkv) + (size_t)3 * D * D);
        g.heads = c.num_heads; g.head_dim = h->hd; g.T = T; g.q = w.q; g.k = w.k; g.vt = w.vt;
        HIP_TRY(launch_gemm_fp8(g, s));
        HIP_TRY(launch_dit_attention(h->cmode, w.q, w.k, w.vt, w.att, B, c.num_heads, h->hd, T, 0, s));
    }
    HIP_TRY(launch_quant_rows_fp8(1, w.att, w.y8, w.ys, ntok, D, s));
    if ((rc = dit_gemm_fp8(h, w.y8, w.ys, D, b.p_proj, h->P(b.proj_b), D, xn, B, s, 0, mod + 2 * D, mstride, x))) return rc;  // x + gate * attn
    std::swap(x, xn);
    HIP_TRY(launch_dit_ln_modulate_fp8(D, x, mod, mstride, 3 * D, 4 * D, w.y8, w.ys, ntok, T, s));
    if ((rc = dit_gemm_fp8(h, w.y8, w.ys, D, b.p_fc1, h->P(b.fc1_b), h->Hd, w.hid, B, s, 1))) return rc;  // GELU(tanh)
    HIP_TRY(launch_quant_rows_fp8(1, w.hid, w.hid8, w.hs, ntok, h->Hd, s));
    if ((rc = dit_gemm_fp8(h, w.hid8, w.hs, h->Hd, b.p_fc2, h->P(b.fc2_b), D, xn, B, s, 0, mod + 5 * D, mstride, x))) return rc;
    std::swap(x, xn);
    return FG_OK;
}

// feat_blocks / feats (nullable): block indices (ascending) whose output tokens [B, T, D] are copied out as fp32 (`features`,
// DiT/network.py:536-540); early: return once the last of them is written (`return_features_early`, :542-543; out then unused)
int dit_forward(fg_dit* h, const float* x_t, const float* t, const float* r, const int64_t* cls, float* out, float* cond_out, int B, DitWs& w,
                hipStream_t s, const int* feat_blocks = nullptr, float* const* feats = nullptr, int nfeat = 0, bool early = false) {
    const fg_dit_config& c = h->cfg;
    const int D = h->D, T = h->T, ntok = B * T;
    const size_t lo_off = (size_t)ntok * D + 32 * (size_t)T;  // bf16x3: elements between the hi and lo planes of q / k / v^T
    // conditioning vector c = t_emb + y_emb + r_emb (:514-533)
    HIP_TRY(launch_dit_fourier(t, w.tf, B, 256, s));
    HIP_TRY(launch_linear(w.tf, h->P(h->tw0), h->P(h->tb0), w.th, B, 256, D, 1, s));
    HIP_TRY(launch_linear(w.th, h->P(h->tw2), h->P(h->tb2), w.temb, B, D, D, 0, s));
    const float* remb = nullptr;
    if (c.r_timestep && r) {
        HIP_TRY(launch_dit_fourier(r, w.tf, B, 256, s));
        HIP_TRY(launch_linear(w.tf, h->P(h->rw0), h->P(h->rb0), w.th, B, 256, D, 1, s));
        HIP_TRY(launch_linear(w.th, h->P(h->rw2), h->P(h->rb2), w.remb, B, D, D, 0, s));
        remb = w.remb;
    }
    HIP_TRY(launch_dit_cond(w.temb, remb, h->P(h->ytab), cls, w.c, w.sc, B, D, c.embedding_rows, h->err_dev, s));
    if (cond_out) HIP_TRY(hipMemcpyAsync(cond_out, w.c, sizeof(float) * (size_t)B * D, hipMemcpyDeviceToDevice, s));
    // tokens
    HIP_TRY(launch_dit_patch_embed(h->dtype, x_t, h->P(h->xw), h->P(h->xb), h->P(h->pos), w.x0, B, c.in_channels, h->grid, c.patch_size, D, s));
    void *x = w.x0, *xn = w.x1;
    // {shift, scale, gate} x {attention, feed-forward} = conditioning_net(c).chunk(6) (:186-187).  bf16 mode at B >= 256: the 28 blocks'
    // Linear(D, 6 D) of silu(c) as ONE token GEMM over the stacked weights (bf16 operands as under the reference's autocast, fp32 out)
    const bool mod_once = h->p_modw && B >= 256;
    const int mstride = mod_once ? (int)h->blocks.size() * 6 * D : 6 * D;
    if (mod_once) {
        HIP_TRY(launch_cvt_rows_bf16(w.sc, w.scb, (int64_t)B * D, s));
        GemmArgs g;
        g.A = w.scb; g.W = h->p_modw; g.bias = h->modb; g.out = w.mod_all; g.M = B; g.N = mstride; g.K = D; g.out_f32 = 1;
        HIP_TRY(launch_gemm_bf16(g, s));
    }
    int bi = 0, blk_idx = 0, fi = 0;
    for (const fg_dit::Blk& b : h->blocks) {
        float* mod = mod_once ? w.mod_all + (size_t)(bi++) * 6 * D : w.mod;
        if (!mod_once) HIP_TRY(launch_linear(w.sc, h->P(b.mod_w), h->P(b.mod_b), w.mod, B, D, 6 * D, 0, s));
        if (h->fp8) {
            const int rc8 = dit_block_fp8(h, b, mod, mstride, x, xn, B, w, s);
            if (rc8) return rc8;
            if (fi < nfeat && feat_blocks[fi] == blk_idx) {
                HIP_TRY(launch_from_act(h->dtype, x, feats[fi], (int64_t)ntok * D, s));
                if (++fi == nfeat && early) return FG_OK;
            }
            ++blk_idx;
            continue;
        }
        if (h->gemm3) HIP_TRY(launch_dit_ln_modulate_split(D, (const float*)x, mod, mstride, 0, D, w.y, ntok, T, s));
        else HIP_TRY(launch_dit_ln_modulate(h->dtype, D, x, mod, mstride, 0, D, w.y, ntok, T, s));
        const bool fa = h->gemm && h->hd == 72;  // qkv stays token-major; attention on wan.hip's LDS-staged kernel
        if (fa) {
            int rc = dit_gemm(h, w.y, D, b.p_qkv, h->P(b.qkv_b), 3 * D, w.qkv, B, s);
            if (rc) return rc;
        } else if (h->gemm3) {
            GemmArgs g;
            g.A = w.y; g.W = b.p_qkv; g.bias = h->P(b.qkv_b); g.M = ntok; g.N = 3 * D; g.K = D;
            g.heads = c.num_heads; g.head_dim = h->hd; g.T = T; g.q = w.q; g.k = w.k; g.vt = w.vt; g.lo_off = lo_off;
            HIP_TRY(launch_gemm_x3(g, 0, s));
        } else if (h->gemm) {
            GemmArgs g;
            g.A = w.y; g.W = b.p_qkv; g.bias = h->P(b.qkv_b); g.M = ntok; g.N = 3 * D; g.K = D;
            g.heads = c.num_heads; g.head_dim = h->hd; g.T = T; g.q = w.q; g.k = w.k; g.vt = w.vt;
            HIP_TRY(launch_gemm_bf16(g, s));
        } else {   // qkv projection, written head-split: q | k [B][H][T][hd], v^T [B][H][hd][T]
            ConvArgs a{};
            a.src1 = w.y; a.C1 = D; a.Hs = a.Ws = a.H = a.W = 16; a.B = B;
            a.wpack = b.p_qkv; a.bias = h->P(b.qkv_b); a.scale = 1.0f; a.Cout = 3 * D;
            a.heads = c.num_heads; a.head_dim = h->hd; a.q_out = w.q; a.k_out = w.k; a.vt_out = w.vt;
            a.heads_lo_off = lo_off;
            HIP_TRY(launch_conv_fused(h->cmode, 1, PRO_NONE, RES_NONE, OUT_HEADS, a, s));
        }
        if (fa) {
            const __bf16* qkv = (const __bf16*)w.qkv;
            HIP_TRY(launch_fa(72, qkv, 3 * D, (int64_t)T * 3 * D, qkv + D, qkv + 2 * D, 3 * D, (int64_t)T * 3 * D, w.att, D, (int64_t)T * D, B,
                              c.num_heads, T, T, s));
        } else {
            HIP_TRY(launch_dit_attention(h->cmode, w.q, w.k, w.vt, w.att, B, c.num_heads, h->hd, T, lo_off, s));
        }
        const void* att = w.att;
        if (h->gemm3) {  // the attention output (fp32) as planes, in the buffer the qkv projection has consumed
            HIP_TRY(launch_split_planes((const float*)w.att, w.y, (int64_t)ntok, D, s));
            att = w.y;
        }
        int rc = dit_gemm(h, att, D, b.p_proj, h->P(b.proj_b), D, xn, B, s, 0, mod + 2 * D, mstride, x);  // x + gate * attn (:192)
        if (rc) return rc;
        std::swap(x, xn);
        if (h->gemm3) HIP_TRY(launch_dit_ln_modulate_split(D, (const float*)x, mod, mstride, 3 * D, 4 * D, w.y, ntok, T, s));
        else HIP_TRY(launch_dit_ln_modulate(h->dtype, D, x, mod, mstride, 3 * D, 4 * D, w.y, ntok, T, s));
        if ((rc = dit_gemm(h, w.y, D, b.p_fc1, h->P(b.fc1_b), h->Hd, w.hid, B, s, 1))) return rc;  // GELU(tanh)
        if ((rc = dit_gemm(h, w.hid, h->Hd, b.p_fc2, h->P(b.fc2_b), D, xn, B, s, 0, mod + 5 * D, mstride, x))) return rc;  // :198
        std::swap(x, xn);
        if (fi < nfeat && feat_blocks[fi] == blk_idx) {
            HIP_TRY(launch_from_act(h->dtype, x, feats[fi], (int64_t)ntok * D, s));
            if (++fi == nfeat && early) return FG_OK;
        }
        ++blk_idx;
    }
    HIP_TRY(launch_linear(w.sc, h->P(h->fmw), h->P(h->fmb), w.fmod, B, D, 2 * D, 0, s));
    HIP_TRY(launch_dit_final(h->dtype, D, x, w.fmod, h->P(h->fw), h->P(h->fb), out, ntok, h->grid, c.patch_size, c.in_channels, s));
    return FG_OK;
}

// ---- forward-mode derivative (fg_dit_jvp): split-bf16 mode, 256 tokens -------------------------------------------------------------
// The primal stream x and the tangent stream xd side by side, both fp32 (kernels: dit_jvp.hip; formulas: DESIGN.md "DiT jvp").  Its own
// workspace plan: the tangent twins of dit_plan's token buffers, the un-gated output h of proj / fc2 and the fc1 pre-activation.
struct DitJvpWs {
    float *zero, *tf, *tfd, *pre, *pred, *th, *thd, *temb, *tembd, *remb, *rembd, *c, *sc, *scd, *mod, *modd, *fmod, *fmodd;
    float *x0, *x1, *xd0, *xd1, *att, *attd, *hid, *hidd;
    void *y, *yd, *q, *k, *vt, *qd, *kd, *vtd, *a, *ad;
};

bool dit_has_jvp(const fg_dit* h) { return h->cmode == FG_DTYPE_BF16X3 && !h->fp8 && h->grid == 16; }

size_t dit_jvp_plan(const fg_dit* h, int B, Arena& A, DitJvpWs& w) {
    const size_t D = h->D, Hd = h->Hd, ntok = (size_t)B * h->T;
    w.zero = A.get<float>((size_t)B);
    w.tf = A.get<float>((size_t)B * 256);
    w.tfd = A.get<float>((size_t)B * 256);
    float** rows[] = {&w.pre, &w.pred, &w.th, &w.thd, &w.temb, &w.tembd, &w.remb, &w.rembd, &w.c, &w.sc, &w.scd};
    for (float** r : rows) *r = A.get<float>((size_t)B * D);
    w.mod = A.get<float>((size_t)B * 6 * D);
    w.modd = A.get<float>((size_t)B * 6 * D);
    w.fmod = A.get<float>((size_t)B * 2 * D);
    w.fmodd = A.get<float>((size_t)B * 2 * D);
    float** toks[] = {&w.x0, &w.x1, &w.xd0, &w.xd1, &w.att, &w.attd};
    for (float** t : toks) *t = A.get<float>(ntok * D);
    w.y = A.take(ntok * D * 4);   // [hi | lo] planes: the bytes of the fp32 tensor
    w.yd = A.take(ntok * D * 4);
    void** heads[] = {&w.q, &w.k, &w.vt, &w.qd, &w.kd, &w.vtd};
    for (void** p : heads) *p = A.take(2 * (ntok * D + 32 * (size_t)h->T) * 2);  // hi and lo planes, 32 rows of slack behind the last head each
    w.hid = A.get<float>(ntok * Hd);
    w.hidd = A.get<float>(ntok * Hd);
    w.a = A.take(ntok * Hd * 4);
    w.ad = A.take(ntok * Hd * 4);
    return (A.off + 255) & ~(size_t)255;
}

// FourierTimeEmbedding with tangent: emb = W2 silu(W0 f(t) + b0) + b2, embd = W2 (silu'(.) o (W0 fd))
int dit_jvp_embed(fg_dit* h, const float* t, const float* td, int w0, int b0, int w2, int b2, float* emb, float* embd, int B, DitJvpWs& w,
                  hipStream_t s) {
    const int D = h->D;
    HIP_TRY(launch_dit_fourier_jvp(t, td, w.tf, w.tfd, B, 256, s));
    HIP_TRY(launch_linear(w.tf, h->P(w0), h->P(b0), w.pre, B, 256, D, 0, s));
    HIP_TRY(launch_linear(w.tfd, h->P(w0), nullptr, w.pred, B, 256, D, 0, s));
    HIP_TRY(launch_dit_silu_jvp(w.pre, w.pred, nullptr, w.th, w.thd, B * D, s));
    HIP_TRY(launch_linear(w.th, h->P(w2), h->P(b2), emb, B, D, D, 0, s));
    HIP_TRY(launch_linear(w.thd, h->P(w2), nullptr, embd, B, D, D, 0, s));
    return FG_OK;
}

int dit_jvp(fg_dit* h, const float* x_t, const float* t, const float* r, const int64_t* cls, const float* vx, const float* vt, const float* vr,
            float* out, float* jvp, int B, DitJvpWs& w, hipStream_t s) {
    const fg_dit_config& c = h->cfg;
    const int D = h->D, Hd = h->Hd, T = h->T, ntok = B * T;
    const size_t lo_off = (size_t)ntok * D + 32 * (size_t)T;
    int rc;
    HIP_TRY(hipMemsetAsync(w.zero, 0, sizeof(float) * (size_t)B, s));
    // conditioning: c = t_emb + y + r_emb, cd = t_embd + r_embd; the blocks read silu(c) and its tangent silu'(c) o cd
    if ((rc = dit_jvp_embed(h, t, vt ? vt : w.zero, h->tw0, h->tb0, h->tw2, h->tb2, w.temb, w.tembd, B, w, s))) return rc;
    const bool has_r = c.r_timestep && r;
    if (has_r && (rc = dit_jvp_embed(h, r, vr ? vr : w.zero, h->rw0, h->rb0, h->rw2, h->rb2, w.remb, w.rembd, B, w, s))) return rc;
    HIP_TRY(launch_dit_cond(w.temb, has_r ? w.remb : nullptr, h->P(h->ytab), cls, w.c, w.sc, B, D, c.embedding_rows, h->err_dev, s));
    HIP_TRY(launch_dit_silu_jvp(w.c, w.tembd, has_r ? w.rembd : nullptr, nullptr, w.scd, B * D, s));
    // tokens: the patch embedding is linear - the tangent stream is the bare convolution of vx
    HIP_TRY(launch_dit_patch_embed(0, x_t, h->P(h->xw), h->P(h->xb), h->P(h->pos), w.x0, B, c.in_channels, h->grid, c.patch_size, D, s));
    HIP_TRY(launch_dit_patch_embed(0, vx, h->P(h->xw), nullptr, nullptr, w.xd0, B, c.in_channels, h->grid, c.patch_size, D, s));
    float *x = w.x0, *xn = w.x1, *xd = w.xd0, *xdn = w.xd1;
    const int ms = 6 * D;
    auto gemm = [&](const void* A, int K, const void* W, const float* bias, int N, void* o, const float* gate, const void* resid) {
        GemmArgs g;
        g.A = A; g.W = W; g.bias = bias; g.out = o; g.M = ntok; g.N = N; g.K = K;
        g.gate = gate; g.gate_stride = ms; g.gate_rows = T; g.resid = resid;
        return launch_gemm_x3(g, 0, s);
    };
    auto qkv = [&](const void* A, const fg_dit::Blk& b, const float* bias, void* q, void* k, void* v) {
        GemmArgs g;
        g.A = A; g.W = b.p_qkv; g.bias = bias; g.M = ntok; g.N = 3 * D; g.K = D;
        g.heads = c.num_heads; g.head_dim = h->hd; g.T = T; g.q = q; g.k = k; g.vt = v; g.lo_off = lo_off;
        return launch_gemm_x3(g, 0, s);
    };
    for (const fg_dit::Blk& b : h->blocks) {
        // {shift, scale, gate} x {attention, feed-forward} and their tangents: modd = W_mod (silu'(c) o cd), no bias
        HIP_TRY(launch_linear(w.sc, h->P(b.mod_w), h->P(b.mod_b), w.mod, B, D, 6 * D, 0, s));
        HIP_TRY(launch_linear(w.scd, h->P(b.mod_w), nullptr, w.modd, B, D, 6 * D, 0, s));
        // attention branch
        HIP_TRY(launch_dit_ln_modulate_jvp(D, x, xd, w.mod, w.modd, ms, 0, D, w.y, w.yd, ntok, T, s));
        HIP_TRY(qkv(w.y, b, h->P(b.qkv_b), w.q, w.k, w.vt));
        HIP_TRY(qkv(w.yd, b, nullptr, w.qd, w.kd, w.vtd));
        HIP_TRY(launch_dit_attention_jvp(w.q, w.k, w.vt, w.qd, w.kd, w.vtd, w.att, w.attd, B, c.num_heads, h->hd, T, lo_off, s));
        HIP_TRY(launch_split_planes(w.att, w.y, (int64_t)ntok, D, s));
        HIP_TRY(launch_split_planes(w.attd, w.yd, (int64_t)ntok, D, s));
        // x' = x + g o h, xd' = xd + g o (W od) + gd o h with h = W o + b: h un-gated (in att's space, consumed above), the middle term
        // on the GEMM's gate + residual epilogue, the outer ones in one elementwise pass
        HIP_TRY(gemm(w.y, D, b.p_proj, h->P(b.proj_b), D, w.att, nullptr, nullptr));
        HIP_TRY(gemm(w.yd, D, b.p_proj, nullptr, D, xdn, w.mod + 2 * D, xd));
        HIP_TRY(launch_dit_gate_update(w.att, w.mod + 2 * D, w.modd + 2 * D, ms, T, x, xn, xdn, (int64_t)ntok, D, s));
        std::swap(x, xn);
        std::swap(xd, xdn);
        // feed-forward branch: fc1 keeps its pre-activation, GELU and its derivative in one pass of their own
        HIP_TRY(launch_dit_ln_modulate_jvp(D, x, xd, w.mod, w.modd, ms, 3 * D, 4 * D, w.y, w.yd, ntok, T, s));
        HIP_TRY(gemm(w.y, D, b.p_fc1, h->P(b.fc1_b), Hd, w.hid, nullptr, nullptr));
        HIP_TRY(gemm(w.yd, D, b.p_fc1, nullptr, Hd, w.hidd, nullptr, nullptr));
        HIP_TRY(launch_dit_gelu_jvp(w.hid, w.hidd, w.a, w.ad, (int64_t)ntok, Hd, s));
        HIP_TRY(gemm(w.a, Hd, b.p_fc2, h->P(b.fc2_b), D, w.att, nullptr, nullptr));
        HIP_TRY(gemm(w.ad, Hd, b.p_fc2, nullptr, D, xdn, w.mod + 5 * D, xd));
        HIP_TRY(launch_dit_gate_update(w.att, w.mod + 5 * D, w.modd + 5 * D, ms, T, x, xn, xdn, (int64_t)ntok, D, s));
        std::swap(x, xn);
        std::swap(xd, xdn);
    }
    HIP_TRY(launch_linear(w.sc, h->P(h->fmw), h->P(h->fmb), w.fmod, B, D, 2 * D, 0, s));
    HIP_TRY(launch_linear(w.scd, h->P(h->fmw), nullptr, w.fmodd, B, D, 2 * D, 0, s));
    HIP_TRY(launch_dit_final_jvp(D, x, xd, w.fmod, w.fmodd, h->P(h->fw), h->P(h->fb), out, jvp, ntok, h->grid, c.patch_size, c.in_channels, s));
    return FG_OK;
}

// fg_dit_pack_group's part: device storage on the first call, then the GEMM weights of the group's blocks
int dit_pack(fg_dit* h, const ParamGroup& in_group, hipStream_t s) {
    const char* e3 = getenv("FASTGEN_AMD_DIT_GEMM3");
    const bool want3 = h->cmode == FG_DTYPE_BF16X3 && !(e3 && e3[0] == '0') && (h->D % 64) == 0 && (h->Hd % 64) == 0 && h->D >= 256;
    // bytes per packed weight element: bf16 2; bf16x3 two bf16 planes = 4, or [hi | lo | hi] = 6 for the split-bf16 token GEMM
    const size_t wsz = h->cmode == FG_DTYPE_BF16 ? 2 : (want3 ? 6 : 4);
    const size_t D = h->D, Hd = h->Hd;
    const char* e1 = getenv("FASTGEN_AMD_DIT_GEMM");
    const bool want1 = h->cmode == FG_DTYPE_BF16 && (h->fp8 || !(e1 && e1[0] == '0')) && (D % 64) == 0 && (Hd % 64) == 0;  // (fp8: fg_dit_create has refused the switch)
    int rc;
    if (!h->device_ready) {
        // (before anything is allocated: a failure here leaves nothing behind for a second attempt to allocate again)
        if (h->grid != 16 && !want1 && !want3)  // conv.hip's token modes are a 16 x 16 image by construction
            return fail(FG_EINVAL, "a %d x %d token grid runs on the token GEMM: FASTGEN_AMD_DIT_GEMM%s=0 excludes it", h->grid, h->grid,
                        h->cmode == FG_DTYPE_BF16X3 ? "3" : "");
        if (h->fp8 && gemm_prepare(4) != 0) return fail(FG_EHIP, "hipFuncSetAttribute(dynamic LDS) failed");
        for (fg_dit::Blk& b : h->blocks) {
            if ((rc = h->alloc(&b.p_qkv, 3 * D * D * wsz)) || (rc = h->alloc(&b.p_proj, D * D * wsz)) ||
                (rc = h->alloc(&b.p_fc1, Hd * D * wsz)) || (rc = h->alloc(&b.p_fc2, D * Hd * wsz)))
                return rc;
        }
        for (size_t i = 0; i < h->params.size(); ++i)
            if (!h->pack_only[i] && !h->is_logvar((int)i) && (rc = h->alloc((void**)&h->own[i], sizeof(float) * (size_t)h->params[i].numel))) return rc;
        if (conv_prepare_all(h->cmode) != 0) return fail(FG_EHIP, "hipFuncSetAttribute(dynamic LDS) failed");
        HIP_TRY(hipHostMalloc((void**)&h->err_host, sizeof(int), hipHostMallocMapped));
        *h->err_host = 0;
        HIP_TRY(hipHostGetDevicePointer((void**)&h->err_dev, h->err_host, 0));
        h->gemm = want1;
        h->gemm3 = want3;
        if ((h->gemm || h->gemm3) && gemm_prepare(3) != 0) return fail(FG_EHIP, "hipFuncSetAttribute(dynamic LDS) failed");
        if (h->gemm && ((rc = h->alloc(&h->p_modw, h->blocks.size() * 6 * D * D * 2)) || (rc = h->alloc((void**)&h->modb, h->blocks.size() * 6 * D * 4))))
            return rc;
        h->device_ready = true;
    }
    size_t bi = 0;
    for (fg_dit::Blk& b : h->blocks) {
        const size_t me = bi++;
        if (!in_group(h->params[b.qkv_w].name)) continue;  // (a block's parameters share their prefix: all of them in the group or none)
        const float *qkv = h->params[b.qkv_w].ptr, *proj = h->params[b.proj_w].ptr, *fc1 = h->params[b.fc1_w].ptr, *fc2 = h->params[b.fc2_w].ptr;
        if (h->gemm3) {
            HIP_TRY(launch_split3_weights(qkv, b.p_qkv, (int)(3 * D), (int)D, s));
            HIP_TRY(launch_split3_weights(proj, b.p_proj, (int)D, (int)D, s));
            HIP_TRY(launch_split3_weights(fc1, b.p_fc1, (int)Hd, (int)D, s));
            HIP_TRY(launch_split3_weights(fc2, b.p_fc2, (int)D, (int)Hd, s));
        } else if (h->gemm) {
            HIP_TRY(launch_cvt_bf16(h->params[b.mod_w].ptr, (__bf16*)h->p_modw + me * 6 * D * D, 6 * D * D, s));
            HIP_TRY(hipMemcpyAsync(h->modb + me * 6 * D, h->params[b.mod_b].ptr, 6 * D * 4, hipMemcpyDeviceToDevice, s));
            if (h->fp8) {  // rows of W [N][K] quantised on the device: e4m3 bytes, then one scale per output channel (inside the bf16-sized allocation)
                auto q8 = [&](const float* wsrc, void* dst, size_t N, size_t K) {
                    return launch_quant_rows_fp8(0, wsrc, dst, reinterpret_cast<float*>(reinterpret_cast<char*>(dst) + N * K), (int64_t)N, (int)K, s);
                };
                HIP_TRY(q8(qkv, b.p_qkv, 3 * D, D));
                HIP_TRY(q8(proj, b.p_proj, D, D));
                HIP_TRY(q8(fc1, b.p_fc1, Hd, D));
                HIP_TRY(q8(fc2, b.p_fc2, D, Hd));
            } else {
                HIP_TRY(launch_cvt_bf16(qkv, b.p_qkv, 3 * D * D, s));
                HIP_TRY(launch_cvt_bf16(proj, b.p_proj, D * D, s));
                HIP_TRY(launch_cvt_bf16(fc1, b.p_fc1, Hd * D, s));
                HIP_TRY(launch_cvt_bf16(fc2, b.p_fc2, D * Hd, s));
            }
        } else {
            HIP_TRY(launch_pack_conv_weights(h->cmode, qkv, b.p_qkv, 3 * h->D, h->D, 1, 0, s));
            HIP_TRY(launch_pack_conv_weights(h->cmode, proj, b.p_proj, h->D, h->D, 1, 0, s));
            HIP_TRY(launch_pack_conv_weights(h->cmode, fc1, b.p_fc1, h->Hd, h->D, 1, 0, s));
            HIP_TRY(launch_pack_conv_weights(h->cmode, fc2, b.p_fc2, h->D, h->Hd, 1, 0, s));
        }
    }
    return FG_OK;
}

}  // namespace

extern "C" {

int fg_dit_create(const fg_dit_config* cfg, fg_dit** out) {
    if (!cfg || !out) return fail(FG_EINVAL, "null argument");
    if (cfg->compute_dtype != FG_DTYPE_F32 && cfg->compute_dtype != FG_DTYPE_BF16 && cfg->compute_dtype != FG_DTYPE_BF16X3 &&
        cfg->compute_dtype != FG_DTYPE_FP8)
        return fail(FG_EINVAL, "bad compute_dtype");
    if (cfg->compute_dtype == FG_DTYPE_FP8 && (cfg->hidden_size <= 0 || cfg->hidden_size % 128 || cfg->mlp_hidden <= 0 || cfg->mlp_hidden % 128))
        return fail(FG_EINVAL, "fp8 mode: hidden_size %d and mlp_hidden %d must be multiples of 128 (the K-step of the e4m3 MFMA)", cfg->hidden_size,
                    cfg->mlp_hidden);
    if (cfg->compute_dtype == FG_DTYPE_FP8) {
        const char* e = getenv("FASTGEN_AMD_DIT_GEMM");
        if (e && e[0] == '0') return fail(FG_EINVAL, "the fp8 mode runs on the token GEMM: FASTGEN_AMD_DIT_GEMM=0 excludes it");
    }
    const int D = cfg->hidden_size;
    if (D != 384 && D != 768 && D != 1024 && D != 1152) return fail(FG_EINVAL, "hidden_size %d unsupported (384, 768, 1024, 1152)", D);
    if (cfg->num_heads <= 0 || D % cfg->num_heads) return fail(FG_EINVAL, "hidden_size must be a multiple of num_heads");
    const int hd = D / cfg->num_heads;
    if (hd != 64 && hd != 72) return fail(FG_EINVAL, "head dim %d unsupported (64, 72)", hd);
    const int grid = cfg->patch_size > 0 && cfg->input_size % cfg->patch_size == 0 ? cfg->input_size / cfg->patch_size : 0;
    if (grid != 16 && grid != 32)
        return fail(FG_EINVAL, "input_size / patch_size must be 16 (256 tokens) or 32 (1024 tokens), got %d / %d", cfg->input_size, cfg->patch_size);
    if (grid != 16 && cfg->compute_dtype == FG_DTYPE_F32)
        return fail(FG_EINVAL, "the exact fp32 mode runs its linears as 16 x 16 token images: a %d x %d token grid excludes it", grid, grid);
    if (cfg->mlp_hidden <= 0 || cfg->mlp_hidden % 128 || cfg->depth <= 0 || cfg->in_channels <= 0 || cfg->embedding_rows <= 0 ||
        cfg->in_channels * cfg->patch_size * cfg->patch_size > 64)
        return fail(FG_EINVAL, "bad depth / mlp_hidden / in_channels / embedding_rows");
    fg_dit* h = new fg_dit();
    h->cfg = *cfg;
    h->fp8 = cfg->compute_dtype == FG_DTYPE_FP8;
    h->cmode = h->fp8 ? FG_DTYPE_BF16 : cfg->compute_dtype;  // (everything but the block linears is the bf16 mode's)
    h->dtype = h->cmode == FG_DTYPE_BF16 ? 1 : 0;
    h->D = D, h->Hd = cfg->mlp_hidden, h->hd = hd, h->grid = grid, h->T = grid * grid;
    const int p = cfg->patch_size, C = cfg->in_channels, PO = p * p * C;
    // module order of the reference's DiT (:233-290); `pos_embed` is its persistent buffer
    h->pos = h->add("pos_embed", {1, h->T, D});
    h->xw = h->add("x_embedder.proj.weight", {D, C, p, p});
    h->xb = h->add("x_embedder.proj.bias", {D});
    h->tw0 = h->add("t_embedder.proj_net.0.weight", {D, 256});
    h->tb0 = h->add("t_embedder.proj_net.0.bias", {D});
    h->tw2 = h->add("t_embedder.proj_net.2.weight", {D, D});
    h->tb2 = h->add("t_embedder.proj_net.2.bias", {D});
    if (cfg->r_timestep) {
        h->rw0 = h->add("r_embedder.proj_net.0.weight", {D, 256});
        h->rb0 = h->add("r_embedder.proj_net.0.bias", {D});
        h->rw2 = h->add("r_embedder.proj_net.2.weight", {D, D});
        h->rb2 = h->add("r_embedder.proj_net.2.bias", {D});
    }
    h->ytab = h->add("y_embedder.class_embeddings.weight", {cfg->embedding_rows, D});
    for (int i = 0; i < cfg->depth; ++i) {
        const std::string b = "blocks." + std::to_string(i) + ".";
        fg_dit::Blk k;
        k.qkv_w = h->add(b + "attention.qkv.weight", {3 * D, D});
        k.qkv_b = h->add(b + "attention.qkv.bias", {3 * D});
        k.proj_w = h->add(b + "attention.proj.weight", {D, D});
        k.proj_b = h->add(b + "attention.proj.bias", {D});
        k.fc1_w = h->add(b + "feed_forward.fc1.weight", {h->Hd, D});
        k.fc1_b = h->add(b + "feed_forward.fc1.bias", {h->Hd});
        k.fc2_w = h->add(b + "feed_forward.fc2.weight", {D, h->Hd});
        k.fc2_b = h->add(b + "feed_forward.fc2.bias", {D});
        k.mod_w = h->add(b + "conditioning_net.1.weight", {6 * D, D});
        k.mod_b = h->add(b + "conditioning_net.1.bias", {6 * D});
        h->blocks.push_back(k);
    }
    h->fw = h->add("final_layer.projection.weight", {PO, D});
    h->fb = h->add("final_layer.projection.bias", {PO});
    h->fmw = h->add("final_layer.adaptive_params.1.weight", {2 * D, D});
    h->fmb = h->add("final_layer.adaptive_params.1.bias", {2 * D});
    h->add("logvar_linear.weight", {1, D});
    h->add("logvar_linear.bias", {1});
    h->own.assign(h->params.size(), nullptr);
    h->pack_only.assign(h->params.size(), 0);
    h->dirty.assign(h->params.size(), 1);
    for (const fg_dit::Blk& k : h->blocks) h->pack_only[k.qkv_w] = h->pack_only[k.proj_w] = h->pack_only[k.fc1_w] = h->pack_only[k.fc2_w] = 1;
    *out = h;
    return FG_OK;
}

void fg_dit_destroy(fg_dit* h) {
    if (!h) return;
    h->sampler.release();
    if (h->err_host) (void)hipHostFree(h->err_host);
    delete h;
}

int fg_dit_num_params(const fg_dit* h) { return h ? (int)h->params.size() : 0; }

int fg_dit_param_info(const fg_dit* h, int index, const char** name, int* ndim, int64_t shape[4]) {
    return param_info(h, index, name, ndim, shape);
}

int fg_dit_bind_param(fg_dit* h, const char* name, const float* device_ptr, int64_t numel) {
    int i;
    const int rc = bind_param(h, name, device_ptr, numel, &i);
    if (!rc) h->dirty[i] = 1;
    return rc;
}

int fg_dit_pack_weights(fg_dit* h, void* stream) { return fg_dit_pack_group(h, "", nullptr, stream); }

// Pack the parameters whose names start with `prefix` (and not with `exclude`, nullable): the unit FSDP2 gathers at a time.
int fg_dit_pack_group(fg_dit* h, const char* prefix, const char* exclude, void* stream) {
    return pack_group(h, prefix, exclude, stream, dit_pack);
}

size_t fg_dit_workspace_bytes(const fg_dit* h, int batch) {
    if (!h || batch <= 0) return 0;
    Arena A;
    A.dry = true;
    DitWs w;
    return dit_plan(h, batch, A, w);
}

int fg_dit_forward(fg_dit* h, const float* x_t, const float* t, const float* r, const int64_t* class_ids, float* out, float* cond_out,
                   int batch, void* workspace, size_t workspace_bytes, void* stream) {
    return fg_dit_forward_features(h, x_t, t, r, class_ids, out, cond_out, nullptr, nullptr, 0, batch, workspace, workspace_bytes, stream);
}

int fg_dit_forward_features(fg_dit* h, const float* x_t, const float* t, const float* r, const int64_t* class_ids, float* out, float* cond_out,
                            const int* feature_blocks, float* const* features, int num_features, int batch, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (!h || !x_t || !t || !class_ids) return fail(FG_EINVAL, "null argument");
    if (num_features < 0 || (num_features > 0 && (!feature_blocks || !features))) return fail(FG_EINVAL, "bad feature arguments");
    for (int i = 0; i < num_features; ++i)
        if (feature_blocks[i] < 0 || feature_blocks[i] >= (int)h->blocks.size() || (i > 0 && feature_blocks[i] <= feature_blocks[i - 1]) || !features[i])
            return fail(FG_EINVAL, "feature_blocks must be ascending block indices in [0, %d) with a buffer each", (int)h->blocks.size());
    if (!out && num_features == 0) return fail(FG_EINVAL, "out == NULL (return the features early) needs at least one feature");
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_dit_pack_weights)");
    if (r && !h->cfg.r_timestep) return fail(FG_EINVAL, "r provided, but the network was built without r_timestep");
    if (batch <= 0 || !workspace || (((uintptr_t)workspace) & 255)) return fail(FG_EINVAL, "bad batch / workspace");
    if (out && out == x_t) return fail(FG_EINVAL, "out must not alias x_t");
    if (h->take_error())
        return fail(FG_EINVAL, "an earlier call on this handle met a class index outside the %d rows of y_embedder.class_embeddings (its output is NaN)",
                    h->cfg.embedding_rows);
    Arena A;
    A.base = (char*)workspace;
    DitWs w;
    const size_t need = dit_plan(h, batch, A, w);
    if (need > workspace_bytes) return fail(FG_ENOMEM, "workspace too small: need %zu bytes for batch %d, got %zu", need, batch, workspace_bytes);
    return dit_forward(h, x_t, t, r, class_ids, out, cond_out, batch, w, (hipStream_t)stream, feature_blocks, features, num_features, out == nullptr);
}

size_t fg_dit_jvp_workspace_bytes(const fg_dit* h, int batch) {
    if (!h || batch <= 0 || !dit_has_jvp(h)) return 0;
    Arena A;
    A.dry = true;
    DitJvpWs w;
    return dit_jvp_plan(h, batch, A, w);
}

int fg_dit_jvp(fg_dit* h, const float* x_t, const float* t, const float* r, const int64_t* class_ids, const float* vx, const float* vt,
               const float* vr, float* out, float* jvp, int batch, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !x_t || !t || !class_ids || !vx || !out || !jvp) return fail(FG_EINVAL, "fg_dit_jvp: null argument");
    if (!dit_has_jvp(h))
        return fail(FG_EINVAL, "fg_dit_jvp: the jvp runs in the bf16x3 compute mode on a 16 x 16 token grid (this handle: compute_dtype %d, %d x %d)",
                    h->cfg.compute_dtype, h->grid, h->grid);
    if (batch <= 0 || (size_t)batch * h->T > (size_t)INT32_MAX) return fail(FG_EINVAL, "fg_dit_jvp: bad batch %d", batch);
    if (!workspace || (((uintptr_t)workspace) & 255)) return fail(FG_EINVAL, "fg_dit_jvp: the workspace must be non-null and 256-byte aligned");
    const size_t img = sizeof(float) * (size_t)batch * h->cfg.in_channels * h->cfg.input_size * h->cfg.input_size;
    auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return b && x < y + nb && y < x + na;
    };
    const size_t vec = sizeof(float) * (size_t)batch;
    for (float* o : {out, jvp})
        if (overlap(o, img, x_t, img) || overlap(o, img, vx, img) || overlap(o, img, t, vec) || overlap(o, img, r, vec) ||
            overlap(o, img, vt, vec) || overlap(o, img, vr, vec) || overlap(o, img, class_ids, sizeof(int64_t) * (size_t)batch) ||
            overlap(o, img, workspace, workspace_bytes))
            return fail(FG_EINVAL, "fg_dit_jvp: out / jvp must not alias an input or the workspace");
    if (overlap(out, img, jvp, img)) return fail(FG_EINVAL, "fg_dit_jvp: out and jvp must not alias each other");
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_dit_pack_weights)");
    if (!h->gemm3) return fail(FG_EINVAL, "fg_dit_jvp: the jvp runs on the split-bf16 token GEMM: FASTGEN_AMD_DIT_GEMM3=0 excludes it");
    if (h->take_error())
        return fail(FG_EINVAL, "an earlier call on this handle met a class index outside the %d rows of y_embedder.class_embeddings (its output is NaN)",
                    h->cfg.embedding_rows);
    Arena A;
    A.base = (char*)workspace;
    DitJvpWs w;
    const size_t need = dit_jvp_plan(h, batch, A, w);
    if (need > workspace_bytes) return fail(FG_ENOMEM, "fg_dit_jvp: workspace too small: need %zu bytes for batch %d, got %zu", need, batch, workspace_bytes);
    return dit_jvp(h, x_t, t, r, class_ids, vx, vt, vr, out, jvp, batch, w, (hipStream_t)stream);
}

// The three new kernels of the jvp on their own (per-op parity tests): every argument is checked before anything is launched.
int fg_op_dit_ln_modulate_jvp(const float* x, const float* xd, const float* mod, const float* modd, int mod_stride, int shift_off, int scale_off,
                              void* y, void* yd, int ntok, int d, int tokens_per_image, void* stream) {
    if (!x || !xd || !mod || !modd || !y || !yd) return fail(FG_EINVAL, "fg_op_dit_ln_modulate_jvp: null pointer");
    if ((((uintptr_t)x) | ((uintptr_t)xd) | ((uintptr_t)mod) | ((uintptr_t)modd) | ((uintptr_t)y) | ((uintptr_t)yd)) & 15)
        return fail(FG_EINVAL, "fg_op_dit_ln_modulate_jvp: tensors must be 16-byte aligned");
    if (ntok <= 0 || tokens_per_image <= 0) return fail(FG_EINVAL, "fg_op_dit_ln_modulate_jvp: ntok %d and tokens_per_image %d must be positive", ntok, tokens_per_image);
    if (d != 384 && d != 768 && d != 1024 && d != 1152) return fail(FG_EINVAL, "fg_op_dit_ln_modulate_jvp: d %d unsupported (384, 768, 1024, 1152)", d);
    if (shift_off < 0 || scale_off < 0 || (mod_stride % 2) || (shift_off % 2) || (scale_off % 2) || mod_stride < shift_off + d || mod_stride < scale_off + d)
        return fail(FG_EINVAL, "fg_op_dit_ln_modulate_jvp: mod_stride / shift_off / scale_off must be even, the offsets + d inside the stride");
    if (y == yd || (const void*)x == y || (const void*)xd == y || (const void*)x == yd || (const void*)xd == yd)
        return fail(FG_EINVAL, "fg_op_dit_ln_modulate_jvp: y / yd must not alias each other or an input");
    HIP_TRY(launch_dit_ln_modulate_jvp(d, x, xd, mod, modd, mod_stride, shift_off, scale_off, y, yd, ntok, tokens_per_image, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_dit_attention_jvp(const void* q, const void* k, const void* vt, const void* qd, const void* kd, const void* vtd, float* out, float* outd,
                            int batch, int heads, int head_dim, int tokens, size_t lo_off, void* stream) {
    if (!q || !k || !vt || !qd || !kd || !vtd || !out || !outd) return fail(FG_EINVAL, "fg_op_dit_attention_jvp: null pointer");
    if (((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)vt) | ((uintptr_t)qd) | ((uintptr_t)kd) | ((uintptr_t)vtd) | ((uintptr_t)out) | ((uintptr_t)outd)) & 15) ||
        (lo_off % 8))
        return fail(FG_EINVAL, "fg_op_dit_attention_jvp: tensors must be 16-byte aligned, lo_off a multiple of 8");
    if (batch <= 0 || heads <= 0 || (head_dim != 64 && head_dim != 72) || (int64_t)batch * heads * 8 > INT32_MAX)
        return fail(FG_EINVAL, "fg_op_dit_attention_jvp: batch and heads > 0 (batch * heads * 8 < 2^31), head_dim 64 or 72 (got %d, %d, %d)", batch, heads,
                    head_dim);
    if (tokens != 256) return fail(FG_EINVAL, "fg_op_dit_attention_jvp: 256 tokens only, got %d", tokens);
    if (lo_off < (size_t)batch * heads * tokens * head_dim + 32 * (size_t)tokens)
        return fail(FG_EINVAL, "fg_op_dit_attention_jvp: lo_off %zu is inside the hi plane (batch * heads * tokens * head_dim + 32 * tokens elements)", lo_off);
    if (out == outd) return fail(FG_EINVAL, "fg_op_dit_attention_jvp: out and outd must not alias");
    HIP_TRY(launch_dit_attention_jvp(q, k, vt, qd, kd, vtd, out, outd, batch, heads, head_dim, tokens, lo_off, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_dit_gelu_jvp(const float* h, const float* hd, void* a, void* ad, int64_t m, int k, void* stream) {
    if (!h || !hd || !a || !ad) return fail(FG_EINVAL, "fg_op_dit_gelu_jvp: null pointer");
    if ((((uintptr_t)h) | ((uintptr_t)hd) | ((uintptr_t)a) | ((uintptr_t)ad)) & 15) return fail(FG_EINVAL, "fg_op_dit_gelu_jvp: tensors must be 16-byte aligned");
    if (m <= 0 || k <= 0 || (k % 4) || m > INT32_MAX || (m * (k / 4) + 255) / 256 > INT32_MAX)
        return fail(FG_EINVAL, "fg_op_dit_gelu_jvp: m %lld > 0, k %d > 0 and a multiple of 4, m k / 1024 < 2^31", (long long)m, k);
    if (a == ad || (const void*)h == a || (const void*)hd == a || (const void*)h == ad || (const void*)hd == ad)
        return fail(FG_EINVAL, "fg_op_dit_gelu_jvp: a / ad must not alias each other or an input");
    HIP_TRY(launch_dit_gelu_jvp(h, hd, a, ad, m, k, (hipStream_t)stream));
    return FG_OK;
}
