// DiT engine (SURVEY §8(f)2): parameter plan with the reference's state-dict names, packed GEMM weights, workspace plan, forward
// orchestration and the C ABI of include/fastgen_amd.h (fg_dit_*).  Textually included by engine.hip inside its `extern "C"` region
// (the handle is a HandleBase; pack_group is engine.hip's).  Reference: fastgen/networks/DiT/network.py:153-201 (DiTBlock),
// :204-225 (OutputProjection), :464-574 (DiT.forward); kernels: dit.hip, gemm.hip + conv.hip's token GEMM modes.
// The four linears of a block (qkv, proj, fc1, fc2) run in one of four flavours (DitFlavour, derived once by dit_flavour).  Everything
// that depends on the flavour is in one place each: dit_linear launches a linear (the only GemmArgs / ConvArgs of a block linear),
// dit_modulate / dit_stage put a token tensor into the flavour's operand form, dit_pack_linear packs a weight; dit_block is the one
// block schedule (dit_forward: modulation vector, dit_block, feature tap), dit_jvp its two-stream twin on the same dit_linear.
}  // extern "C" (reopened below: the structures and helpers are C++)

// How the four block linears run.  The rest of the network follows cmode: the token tensors, attention, patch embedding, final layer.
enum DitFlavour {
    DIT_CONV,  // conv.hip's 16 x 16 token modes in cmode's arithmetic: the exact fp32 mode; bf16 / bf16x3 with their switch at 0
    DIT_BF16,  // gemm.hip on plain [N][K] bf16 weights
    DIT_X3,    // gemm.hip's split-bf16 flavour: [hi | lo | hi] weights, [hi | lo] activation planes
    DIT_FP8,   // gemm.hip on e4m3 operands, the weight as [N][K] e4m3fn bytes followed by the N fp32 channel scales; cmode bf16
};
enum { DIT_QKV, DIT_PROJ, DIT_FC1, DIT_FC2, DIT_NLIN };  // the block linears, in the reference's module order

struct fg_dit : HandleBase {
    fg_dit_config cfg;
    int dtype = 0, cmode = 0;  // as fg_edm: storage of the token tensors (0 fp32 / 1 bf16), arithmetic of the GEMMs (FG_DTYPE_*)
    DitFlavour flavour = DIT_CONV;
    int D = 0, Hd = 0, hd = 0, T = 0, grid = 0;  // hidden size, MLP hidden size, head dim, tokens per image, patches per side
    struct Lin {  // one block linear: parameter indices of weight [N][K] and bias [N], the weight packed for the flavour (owned)
        int w = -1, b = -1, N = 0, K = 0;
        void* p = nullptr;
    };
    struct Blk {
        Lin lin[DIT_NLIN];
        int mod_w, mod_b;
    };
    std::vector<Blk> blocks;
    int pos = -1, xw = -1, xb = -1, tw0 = -1, tb0 = -1, tw2 = -1, tb2 = -1, rw0 = -1, rb0 = -1, rw2 = -1, rb2 = -1, ytab = -1, fw = -1, fb = -1,
        fmw = -1, fmb = -1;
    void* p_modw = nullptr;   // DIT_BF16 / DIT_FP8: all blocks' conditioning_net weights stacked [depth * 6 D][D] bf16 ...
    float* modb = nullptr;    // ... and their biases [depth * 6 D]: one GEMM per forward instead of one 256-row linear per block
    bool bf16_gemm() const { return flavour == DIT_BF16 || flavour == DIT_FP8; }  // (what the two share: p_modw, token-major qkv at head dim 72)
    SamplerCache sampler;  // fg_dit_sampler_run (engine_sampler.inc)
    // a kernel that met an out-of-range class index raises *err_host (pinned, mapped: err_dev is its device address); the next call on
    // the handle reports it (the reference's nn.Embedding device-asserts; nothing is clamped, the sample's output is NaN)
    int *err_host = nullptr, *err_dev = nullptr;
    int take_error() {
        if (!err_host || !*err_host) return 0;
        *err_host = 0;
        return 1;
    }
    // Parameters as the kernels read them.  The four block linears are read from the caller's tensors at PACK time only (into the
    // flavour's layout, Lin::p); every other parameter is copied into `own` at pack time, so that between two packs nothing points into
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
    void *y8, *hid8;   // DIT_FP8: the quantised A operands [ntok][D] / [ntok][Hd] ...
    float *ys, *hs;    // ... and their per-token scales
};

size_t dit_plan(const fg_dit* h, int B, Arena& A, DitWs& w) {
    const size_t tsz = h->dtype ? 2 : 4;
    const size_t D = h->D, ntok = (size_t)B * h->T;
    const bool fp8 = h->flavour == DIT_FP8;
    w.tf = A.get<float>((size_t)B * 256);
    w.th = A.get<float>((size_t)B * D);
    w.temb = A.get<float>((size_t)B * D);
    w.remb = A.get<float>((size_t)B * D);
    w.c = A.get<float>((size_t)B * D);
    w.sc = A.get<float>((size_t)B * D);
    w.mod = A.get<float>((size_t)B * 6 * D);
    w.mod_all = A.get<float>(h->bf16_gemm() && B >= 256 ? (size_t)B * h->blocks.size() * 6 * D : 0);
    w.scb = A.take(h->bf16_gemm() && B >= 256 ? (size_t)B * D * 2 : 0);
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
    w.qkv = A.take(ntok * 3 * D * tsz);  // token-major q | k | v of the LDS-staged attention (DIT_BF16 / DIT_FP8, head dim 72)
    w.y8 = A.take(fp8 ? ntok * D : 0);
    w.hid8 = A.take(fp8 ? ntok * (size_t)h->Hd : 0);
    w.ys = A.get<float>(fp8 ? ntok : 0);
    w.hs = A.get<float>(fp8 ? ntok : 0);
    return (A.off + 255) & ~(size_t)255;
}

// A block linear's input in the handle's flavour: a token tensor in cmode's storage (DIT_CONV, DIT_BF16), [hi | lo] planes (DIT_X3),
// or e4m3 bytes with their per-token scales (DIT_FP8)
struct DitOperand {
    const void* p = nullptr;
    const float* scale = nullptr;
};

// ... and where its result goes: the token epilogue out[tok][n] = resid + gate * act(acc + bias) (dit_tok), or the head-split one
// q | k [B][H][T][hd], v^T [B][H][hd][T], the lo planes of the bf16x3 mode lo_off elements behind (dit_heads)
struct DitEpilogue {
    void* out = nullptr;
    int act = 0;
    const float* gate = nullptr;
    int gate_stride = 0;
    const void* resid = nullptr;
    void *q = nullptr, *k = nullptr, *vt = nullptr;
    size_t lo_off = 0;
};
DitEpilogue dit_tok(void* out, int act = 0, const float* gate = nullptr, int gate_stride = 0, const void* resid = nullptr) {
    DitEpilogue e;
    e.out = out, e.act = act, e.gate = gate, e.gate_stride = gate_stride, e.resid = resid;
    return e;
}
DitEpilogue dit_heads(void* q, void* k, void* vt, size_t lo_off) {
    DitEpilogue e;
    e.q = q, e.k = k, e.vt = vt, e.lo_off = lo_off;
    return e;
}

// One block linear in the handle's flavour: epilogue(sum_k a[tok][k] W[n][k] + bias[n]) over B * T tokens (bias nullable: the tangent
// stream of dit_jvp)
int dit_linear(const fg_dit* h, DitOperand a, const fg_dit::Lin& l, const float* bias, const DitEpilogue& e, int B, hipStream_t s) {
    if (h->flavour == DIT_CONV) {
        ConvArgs c{};
        c.src1 = a.p; c.C1 = l.K; c.Hs = c.Ws = c.H = c.W = 16; c.B = B;
        c.wpack = l.p; c.bias = bias; c.scale = 1.0f; c.Cout = l.N;
        c.out = e.out; c.act = e.act; c.gate = e.gate; c.gate_stride = e.gate_stride; c.resid = e.resid;
        if (e.q) c.heads = h->cfg.num_heads, c.head_dim = h->hd, c.q_out = e.q, c.k_out = e.k, c.vt_out = e.vt, c.heads_lo_off = e.lo_off;
        HIP_TRY(launch_conv_fused(h->cmode, 1, PRO_NONE, RES_NONE, e.q ? OUT_HEADS : OUT_TOK, c, s));
        return FG_OK;
    }
    GemmArgs g;
    g.A = a.p; g.W = l.p; g.bias = bias; g.M = B * h->T; g.N = l.N; g.K = l.K;
    if (e.q) g.heads = h->cfg.num_heads, g.head_dim = h->hd, g.T = h->T, g.q = e.q, g.k = e.k, g.vt = e.vt;
    else g.out = e.out, g.act = e.act, g.gate = e.gate, g.gate_stride = e.gate_stride, g.gate_rows = h->T, g.resid = e.resid;
    if (h->flavour == DIT_X3) {  // a GELU'd output (fc1) is written as the [hi | lo] planes fc2 reads, every other one as fp32
        g.lo_off = e.lo_off;
        HIP_TRY(launch_gemm_x3(g, e.act ? 1 : 0, s));
    } else if (h->flavour == DIT_FP8) {  // (the channel scales lie behind the packed bytes: dit_pack_linear)
        g.a_scale = a.scale;
        g.w_scale = reinterpret_cast<const float*>(reinterpret_cast<const char*>(l.p) + (size_t)l.N * l.K);
        HIP_TRY(launch_gemm_fp8(g, s));
    } else {
        HIP_TRY(launch_gemm_bf16(g, s));
    }
    return FG_OK;
}

// LayerNorm-modulate of the stream x as the flavour's operand: y = LN(x) (1 + mod[scale_off ...]) + mod[shift_off ...]
int dit_modulate(const fg_dit* h, const void* x, const float* mod, int mstride, int shift_off, int scale_off, int ntok, DitWs& w, hipStream_t s,
                 DitOperand& y) {
    y = DitOperand{w.y, nullptr};
    if (h->flavour == DIT_FP8) {
        y = DitOperand{w.y8, w.ys};
        HIP_TRY(launch_dit_ln_modulate_fp8(h->D, x, mod, mstride, shift_off, scale_off, w.y8, w.ys, ntok, h->T, s));
    } else if (h->flavour == DIT_X3) {
        HIP_TRY(launch_dit_ln_modulate_split(h->D, (const float*)x, mod, mstride, shift_off, scale_off, w.y, ntok, h->T, s));
    } else {
        HIP_TRY(launch_dit_ln_modulate(h->dtype, h->D, x, mod, mstride, shift_off, scale_off, w.y, ntok, h->T, s));
    }
    return FG_OK;
}

// A token tensor [ntok][K] that a kernel left in cmode's storage (the attention output, the hidden layer) as the flavour's operand:
// as it is, as planes in `planes` (nullptr: src holds planes already), or quantised into q8 / scale.  The rows of both tensors cross
// their producing kernels' tiles, so the quantiser is a pass of its own.
int dit_stage(const fg_dit* h, const void* src, int K, void* planes, void* q8, float* scale, int ntok, hipStream_t s, DitOperand& a) {
    a = DitOperand{src, nullptr};
    if (h->flavour == DIT_X3 && planes) {
        HIP_TRY(launch_split_planes((const float*)src, planes, (int64_t)ntok, K, s));
        a.p = planes;
    } else if (h->flavour == DIT_FP8) {
        HIP_TRY(launch_quant_rows_fp8(1, src, q8, scale, ntok, K, s));
        a = DitOperand{q8, scale};
    }
    return FG_OK;
}

// One transformer block (DiTBlock.forward, :186-199) on the stream x (xn: its other buffer; swapped so that x is the output); mod:
// {shift, scale, gate} x {attention, feed-forward} of stride mstride per sample.  q / k / v, attention and the stream are cmode's.
int dit_block(const fg_dit* h, const fg_dit::Blk& b, const float* mod, int mstride, void*& x, void*& xn, int B, DitWs& w, hipStream_t s) {
    const int D = h->D, T = h->T, ntok = B * T, heads = h->cfg.num_heads;
    DitOperand a;  // the operand the next linear reads
    const auto linear = [&](int l, const DitEpilogue& e) { return dit_linear(h, a, b.lin[l], h->P(b.lin[l].b), e, B, s); };
    int rc;
    if ((rc = dit_modulate(h, x, mod, mstride, 0, D, ntok, w, s, a))) return rc;
    if (h->bf16_gemm() && h->hd == 72) {  // qkv stays token-major; attention on wan.hip's LDS-staged kernel
        if ((rc = linear(DIT_QKV, dit_tok(w.qkv)))) return rc;
        const __bf16* qkv = (const __bf16*)w.qkv;
        HIP_TRY(launch_fa(72, qkv, 3 * D, (int64_t)T * 3 * D, qkv + D, qkv + 2 * D, 3 * D, (int64_t)T * 3 * D, w.att, D, (int64_t)T * D, B, heads, T,
                          T, s));
    } else {  // head-split q | k | v^T; lo_off: elements between their hi and lo planes (only the bf16x3 kernels read it)
        const size_t lo_off = h->flavour == DIT_FP8 ? 0 : (size_t)ntok * D + 32 * (size_t)T;
        if ((rc = linear(DIT_QKV, dit_heads(w.q, w.k, w.vt, lo_off)))) return rc;
        HIP_TRY(launch_dit_attention(h->cmode, w.q, w.k, w.vt, w.att, B, heads, h->hd, T, lo_off, s));
    }
    // x + gate * proj(attention) (:192); bf16x3: its planes go into the buffer the qkv projection has consumed
    if ((rc = dit_stage(h, w.att, D, w.y, w.y8, w.ys, ntok, s, a)) || (rc = linear(DIT_PROJ, dit_tok(xn, 0, mod + 2 * D, mstride, x)))) return rc;
    std::swap(x, xn);
    // x + gate * fc2(GELU(tanh)(fc1(.))) (:198); bf16x3: fc1 writes the hidden layer as planes itself
    if ((rc = dit_modulate(h, x, mod, mstride, 3 * D, 4 * D, ntok, w, s, a)) || (rc = linear(DIT_FC1, dit_tok(w.hid, 1)))) return rc;
    if ((rc = dit_stage(h, w.hid, h->Hd, nullptr, w.hid8, w.hs, ntok, s, a)) || (rc = linear(DIT_FC2, dit_tok(xn, 0, mod + 5 * D, mstride, x)))) return rc;
    std::swap(x, xn);
    return FG_OK;
}

// feat_blocks / feats (nullable): block indices (ascending) whose output tokens [B, T, D] are copied out as fp32 (`features`,
// DiT/network.py:536-540); early: return once the last of them is written (`return_features_early`, :542-543; out then unused)
int dit_forward(fg_dit* h, const float* x_t, const float* t, const float* r, const int64_t* cls, float* out, float* cond_out, int B, DitWs& w,
                hipStream_t s, const int* feat_blocks = nullptr, float* const* feats = nullptr, int nfeat = 0, bool early = false) {
    const fg_dit_config& c = h->cfg;
    const int D = h->D, ntok = B * h->T;
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
    // {shift, scale, gate} x {attention, feed-forward} = conditioning_net(c).chunk(6) (:186-187).  DIT_BF16 / DIT_FP8 at B >= 256: the 28 blocks'
    // Linear(D, 6 D) of silu(c) as ONE token GEMM over the stacked weights (bf16 operands as under the reference's autocast, fp32 out)
    const bool mod_once = h->bf16_gemm() && B >= 256;
    const int mstride = mod_once ? (int)h->blocks.size() * 6 * D : 6 * D;
    if (mod_once) {
        HIP_TRY(launch_cvt_rows_bf16(w.sc, w.scb, (int64_t)B * D, s));
        GemmArgs g;
        g.A = w.scb; g.W = h->p_modw; g.bias = h->modb; g.out = w.mod_all; g.M = B; g.N = mstride; g.K = D; g.out_f32 = 1;
        HIP_TRY(launch_gemm_bf16(g, s));
    }
    int bi = 0, fi = 0;
    for (const fg_dit::Blk& b : h->blocks) {
        float* mod = mod_once ? w.mod_all + (size_t)bi * 6 * D : w.mod;
        if (!mod_once) HIP_TRY(launch_linear(w.sc, h->P(b.mod_w), h->P(b.mod_b), w.mod, B, D, 6 * D, 0, s));
        const int rc = dit_block(h, b, mod, mstride, x, xn, B, w, s);
        if (rc) return rc;
        if (fi < nfeat && feat_blocks[fi] == bi) {
            HIP_TRY(launch_from_act(h->dtype, x, feats[fi], (int64_t)ntok * D, s));
            if (++fi == nfeat && early) return FG_OK;
        }
        ++bi;
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

// (the bf16x3 mode is DIT_X3, or DIT_CONV by its switch: that handle has a jvp plan too, and fg_dit_jvp refuses it by the switch's name)
bool dit_has_jvp(const fg_dit* h) { return h->cmode == FG_DTYPE_BF16X3 && h->grid == 16; }

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
    // a block linear on one stream's operand planes; the tangent stream's has no bias
    auto lin = [&](const void* a, const fg_dit::Lin& l, bool bias, const DitEpilogue& e) {
        return dit_linear(h, DitOperand{a, nullptr}, l, bias ? h->P(l.b) : nullptr, e, B, s);
    };
    for (const fg_dit::Blk& b : h->blocks) {
        const fg_dit::Lin &qkv = b.lin[DIT_QKV], &proj = b.lin[DIT_PROJ], &fc1 = b.lin[DIT_FC1], &fc2 = b.lin[DIT_FC2];
        // {shift, scale, gate} x {attention, feed-forward} and their tangents: modd = W_mod (silu'(c) o cd), no bias
        HIP_TRY(launch_linear(w.sc, h->P(b.mod_w), h->P(b.mod_b), w.mod, B, D, 6 * D, 0, s));
        HIP_TRY(launch_linear(w.scd, h->P(b.mod_w), nullptr, w.modd, B, D, 6 * D, 0, s));
        // attention branch
        HIP_TRY(launch_dit_ln_modulate_jvp(D, x, xd, w.mod, w.modd, ms, 0, D, w.y, w.yd, ntok, T, s));
        if ((rc = lin(w.y, qkv, true, dit_heads(w.q, w.k, w.vt, lo_off))) || (rc = lin(w.yd, qkv, false, dit_heads(w.qd, w.kd, w.vtd, lo_off)))) return rc;
        HIP_TRY(launch_dit_attention_jvp(w.q, w.k, w.vt, w.qd, w.kd, w.vtd, w.att, w.attd, B, c.num_heads, h->hd, T, lo_off, s));
        HIP_TRY(launch_split_planes(w.att, w.y, (int64_t)ntok, D, s));
        HIP_TRY(launch_split_planes(w.attd, w.yd, (int64_t)ntok, D, s));
        // x' = x + g o h, xd' = xd + g o (W od) + gd o h with h = W o + b: h un-gated (in att's space, consumed above), the middle term
        // on the GEMM's gate + residual epilogue, the outer ones in one elementwise pass
        if ((rc = lin(w.y, proj, true, dit_tok(w.att, 0, nullptr, ms))) || (rc = lin(w.yd, proj, false, dit_tok(xdn, 0, w.mod + 2 * D, ms, xd)))) return rc;
        HIP_TRY(launch_dit_gate_update(w.att, w.mod + 2 * D, w.modd + 2 * D, ms, T, x, xn, xdn, (int64_t)ntok, D, s));
        std::swap(x, xn);
        std::swap(xd, xdn);
        // feed-forward branch: fc1 keeps its pre-activation, GELU and its derivative in one pass of their own
        HIP_TRY(launch_dit_ln_modulate_jvp(D, x, xd, w.mod, w.modd, ms, 3 * D, 4 * D, w.y, w.yd, ntok, T, s));
        if ((rc = lin(w.y, fc1, true, dit_tok(w.hid, 0, nullptr, ms))) || (rc = lin(w.yd, fc1, false, dit_tok(w.hidd, 0, nullptr, ms)))) return rc;
        HIP_TRY(launch_dit_gelu_jvp(w.hid, w.hidd, w.a, w.ad, (int64_t)ntok, Hd, s));
        if ((rc = lin(w.a, fc2, true, dit_tok(w.att, 0, nullptr, ms))) || (rc = lin(w.ad, fc2, false, dit_tok(xdn, 0, w.mod + 5 * D, ms, xd)))) return rc;
        HIP_TRY(launch_dit_gate_update(w.att, w.mod + 5 * D, w.modd + 5 * D, ms, T, x, xn, xdn, (int64_t)ntok, D, s));
        std::swap(x, xn);
        std::swap(xd, xdn);
    }
    HIP_TRY(launch_linear(w.sc, h->P(h->fmw), h->P(h->fmb), w.fmod, B, D, 2 * D, 0, s));
    HIP_TRY(launch_linear(w.scd, h->P(h->fmw), nullptr, w.fmodd, B, D, 2 * D, 0, s));
    HIP_TRY(launch_dit_final_jvp(D, x, xd, w.fmod, w.fmodd, h->P(h->fw), h->P(h->fb), out, jvp, ntok, h->grid, c.patch_size, c.in_channels, s));
    return FG_OK;
}

// The flavour of a configuration: the compute mode, moved onto conv.hip's token modes by its switch at 0.  (fg_dit_create's checks of
// hidden_size and mlp_hidden leave nothing for the token GEMMs to refuse, and it refuses the fp8 mode with the switch itself.)
DitFlavour dit_flavour(int compute_dtype) {
    const auto off = [](const char* name) {
        const char* e = getenv(name);
        return e && e[0] == '0';
    };
    if (compute_dtype == FG_DTYPE_FP8) return DIT_FP8;
    if (compute_dtype == FG_DTYPE_BF16 && !off("FASTGEN_AMD_DIT_GEMM")) return DIT_BF16;
    if (compute_dtype == FG_DTYPE_BF16X3 && !off("FASTGEN_AMD_DIT_GEMM3")) return DIT_X3;
    return DIT_CONV;
}

// One block linear's fp32 weight [N][K] into the flavour's layout
int dit_pack_linear(const fg_dit* h, const fg_dit::Lin& l, hipStream_t s) {
    const float* src = h->params[l.w].ptr;
    const size_t n = (size_t)l.N * l.K;
    if (h->flavour == DIT_X3) HIP_TRY(launch_split3_weights(src, l.p, l.N, l.K, s));
    else if (h->flavour == DIT_BF16) HIP_TRY(launch_cvt_bf16(src, l.p, n, s));
    else if (h->flavour == DIT_FP8)  // rows quantised on the device: e4m3 bytes, then one scale per output channel (inside the bf16-sized allocation)
        HIP_TRY(launch_quant_rows_fp8(0, src, l.p, reinterpret_cast<float*>(reinterpret_cast<char*>(l.p) + n), (int64_t)l.N, l.K, s));
    else HIP_TRY(launch_pack_conv_weights(h->cmode, src, l.p, l.N, l.K, 1, 0, s));
    return FG_OK;
}

// fg_dit_pack_group's part: device storage on the first call, then the GEMM weights of the group's blocks
int dit_pack(fg_dit* h, const ParamGroup& in_group, hipStream_t s) {
    const size_t D = h->D, depth = h->blocks.size();
    int rc;
    if (!h->device_ready) {
        // (before anything is allocated: a failure here leaves nothing behind for a second attempt to allocate again)
        if (h->grid != 16 && h->flavour == DIT_CONV)  // conv.hip's token modes are a 16 x 16 image by construction
            return fail(FG_EINVAL, "a %d x %d token grid runs on the token GEMM: FASTGEN_AMD_DIT_GEMM%s=0 excludes it", h->grid, h->grid,
                        h->cmode == FG_DTYPE_BF16X3 ? "3" : "");
        if (h->flavour == DIT_FP8 && gemm_prepare(4) != 0) return fail(FG_EHIP, "hipFuncSetAttribute(dynamic LDS) failed");
        // bytes per packed weight element: bf16 2 (the e4m3 bytes and their scales fit inside); bf16x3 two bf16 planes = 4, or
        // [hi | lo | hi] = 6 for the split-bf16 token GEMM
        const size_t wsz = h->cmode == FG_DTYPE_BF16 ? 2 : (h->flavour == DIT_X3 ? 6 : 4);
        for (fg_dit::Blk& b : h->blocks)
            for (fg_dit::Lin& l : b.lin)
                if ((rc = h->alloc(&l.p, (size_t)l.N * l.K * wsz))) return rc;
        for (size_t i = 0; i < h->params.size(); ++i)
            if (!h->pack_only[i] && !h->is_logvar((int)i) && (rc = h->alloc((void**)&h->own[i], sizeof(float) * (size_t)h->params[i].numel))) return rc;
        if (conv_prepare_all(h->cmode) != 0) return fail(FG_EHIP, "hipFuncSetAttribute(dynamic LDS) failed");
        HIP_TRY(hipHostMalloc((void**)&h->err_host, sizeof(int), hipHostMallocMapped));
        *h->err_host = 0;
        HIP_TRY(hipHostGetDevicePointer((void**)&h->err_dev, h->err_host, 0));
        if (h->flavour != DIT_CONV && gemm_prepare(3) != 0) return fail(FG_EHIP, "hipFuncSetAttribute(dynamic LDS) failed");
        if (h->bf16_gemm() && ((rc = h->alloc(&h->p_modw, depth * 6 * D * D * 2)) || (rc = h->alloc((void**)&h->modb, depth * 6 * D * 4)))) return rc;
        h->device_ready = true;
    }
    for (size_t me = 0; me < depth; ++me) {
        const fg_dit::Blk& b = h->blocks[me];
        if (!in_group(h->params[b.lin[DIT_QKV].w].name)) continue;  // (a block's parameters share their prefix: all of them in the group or none)
        if (h->bf16_gemm()) {
            HIP_TRY(launch_cvt_bf16(h->params[b.mod_w].ptr, (__bf16*)h->p_modw + me * 6 * D * D, 6 * D * D, s));
            HIP_TRY(hipMemcpyAsync(h->modb + me * 6 * D, h->params[b.mod_b].ptr, 6 * D * 4, hipMemcpyDeviceToDevice, s));
        }
        for (const fg_dit::Lin& l : b.lin)
            if ((rc = dit_pack_linear(h, l, s))) return rc;
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
    h->flavour = dit_flavour(cfg->compute_dtype);
    h->cmode = h->flavour == DIT_FP8 ? FG_DTYPE_BF16 : cfg->compute_dtype;  // (everything but the block linears is the bf16 mode's)
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
    const struct {
        const char* name;
        int N, K;
    } lins[DIT_NLIN] = {{"attention.qkv", 3 * D, D}, {"attention.proj", D, D}, {"feed_forward.fc1", h->Hd, D}, {"feed_forward.fc2", D, h->Hd}};
    for (int i = 0; i < cfg->depth; ++i) {
        const std::string b = "blocks." + std::to_string(i) + ".";
        fg_dit::Blk k;
        for (int l = 0; l < DIT_NLIN; ++l) {
            fg_dit::Lin& n = k.lin[l];
            n.N = lins[l].N, n.K = lins[l].K;
            n.w = h->add(b + lins[l].name + ".weight", {n.N, n.K});
            n.b = h->add(b + lins[l].name + ".bias", {n.N});
        }
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
    for (const fg_dit::Blk& k : h->blocks)
        for (const fg_dit::Lin& l : k.lin) h->pack_only[l.w] = 1;
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
    DitWs w;
    const int rc = setup_ws(dit_plan, h, batch, workspace, workspace_bytes, w);  // (its own argument checks have passed above; FG_ENOMEM is left)
    if (rc) return rc;
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
    if (h->flavour != DIT_X3) return fail(FG_EINVAL, "fg_dit_jvp: the jvp runs on the split-bf16 token GEMM: FASTGEN_AMD_DIT_GEMM3=0 excludes it");
    if (h->take_error())
        return fail(FG_EINVAL, "an earlier call on this handle met a class index outside the %d rows of y_embedder.class_embeddings (its output is NaN)",
                    h->cfg.embedding_rows);
    DitJvpWs w;
    const int rc = setup_ws(dit_jvp_plan, h, batch, workspace, workspace_bytes, w);  // (as in fg_dit_forward_features)
    if (rc) return rc;
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
