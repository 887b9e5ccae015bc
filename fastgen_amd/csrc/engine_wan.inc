// Causal video DiT engine (SURVEY 8(f)3 / CausVid row of 8(a)): parameter plan with the state-dict names of the reference's
// CausalWan (`transformer.` + diffusers' WanTransformer3DModel keys), bf16 (fp8 mode: e4m3) weight copies, per-handle KV caches, forward
// orchestration and the C ABI of include/fastgen_amd.h (fg_wan_*); the bidirectional network `Wan` (Wan/network.py: fg_wan_create_ex,
// fg_wan_forward_full) is a mode of the same forward.  Textually included by engine.hip inside its `extern "C"` region
// (the handle is a HandleBase; pack_group is engine.hip's).
// Reference: fastgen/networks/Wan/network_causal.py:467-550 (block), :568-705 (prepare), :815-913 (block loop, cache positions),
// fastgen/networks/Wan/network.py:156-279 (classify_forward); kernels: wan.hip + gemm.hip + dit.hip's LayerNorm-modulate.
}  // extern "C" (reopened below)

struct fg_wan : HandleBase {
    fg_wan_config cfg;
    int D = 0, Fd = 0, H = 0;
    // FG_DTYPE_FP8: the six linears of a block that read the video tokens (p_qkv, p_o, p_q2, p_o2, p_f0, p_f2) hold [N][K] e4m3fn bytes
    // followed by the N fp32 channel scales instead of bf16 (inside the same allocation), and their A operands are quantised per
    // token (wan_modulate / wan_stage); wan_gemm is the one place that launches either.  The text side (p_x1, p_x2, p_kv2) stays bf16.
    bool fp8 = false;
    struct Blk {
        int sst, q_w, q_b, k_w, k_b, v_w, v_b, o_w, o_b, nq, nk;          // attn1
        int q2_w, q2_b, k2_w, k2_b, v2_w, v2_b, o2_w, o2_b, nq2, nk2;      // attn2
        int n2_w, n2_b, f0_w, f0_b, f2_w, f2_b;
        int ak_w = -1, ak_b = -1, av_w = -1, av_b = -1, nak = -1;  // attn2.add_k_proj / add_v_proj / norm_added_k (fg_wan_create_i2v, image_dim > 0)
        void *p_qkv = nullptr, *p_o = nullptr, *p_q2 = nullptr, *p_kv2 = nullptr, *p_o2 = nullptr, *p_f0 = nullptr, *p_f2 = nullptr;  // bf16 [N][K] (fp8: above)
        float *b_qkv = nullptr, *b_kv2 = nullptr, *n2mod = nullptr;  // fused biases; norm2 as {shift = bias, scale = weight - 1}
        void *kc = nullptr, *vc = nullptr;   // self-attention cache [B][cap][D] bf16
        void* kv2 = nullptr;                 // cross-attention cache [B][Lt][2 D] bf16 (k normalised | v)
        void* p_akv = nullptr;               // add_k_proj | add_v_proj, bf16 [2 D][D] in every mode (as p_kv2)
        float* b_akv = nullptr;
        void* kvi = nullptr;                 // image cross-attention cache [B][ceil32(Li)][2 D] bf16 (k normalised | v), zero-filled
        int pin_w = -1, pin_b = -1, pout_w = -1, pout_b = -1;  // a VACE block's proj_in (block 0 only) / proj_out (fg_wan_create_vace)
        void *p_pin = nullptr, *p_pout = nullptr;              // ... bf16 [D][D] in every mode
        // every parameter index of the block (fg_wan_pack_group's all-or-none check on a VACE block)
        template <typename F>
        void each_param(F&& f) const {
            for (int idx : {sst, q_w, q_b, k_w, k_b, v_w, v_b, o_w, o_b, nq, nk, q2_w, q2_b, k2_w, k2_b, v2_w, v2_b, o2_w, o2_b, nq2, nk2, n2_w, n2_b,
                            f0_w, f0_b, f2_w, f2_b, ak_w, ak_b, av_w, av_b, nak, pin_w, pin_b, pout_w, pout_b})
                if (idx >= 0) f(idx);
        }
    };
    std::vector<Blk> blocks;
    // fg_wan_create_vace: the control branch (VaceWan/network.py).  `vblocks` are the VACE blocks - main blocks with their own weights,
    // their own text k / v (kv2) and proj_in / proj_out; no self-attention cache (the bidirectional calls alone serve such a handle).
    // The context (fg_wan_set_vace_context) is `vctx` = proj_in(pad(vace_patch_embedding(vid_context))) [B][L][D] bf16, owned here and
    // rewritten in place while its shape stays (the loops' graphs name it); the hint scales are `vscale` [n][D] fp32, the gate rows of
    // the injection GEMM, rewritten in place too (`vscale_host`: their values, ones until fg_wan_set_vace_scale; the rows exist from
    // the first pack on).
    bool is_vace = false;
    fg_wan_vace_config vace{};
    std::vector<Blk> vblocks;
    int vpe_w = -1, vpe_b = -1;  // vace_patch_embedding
    void* vctx = nullptr;
    int vctx_B = 0, vctx_F = 0, vctx_H = 0, vctx_W = 0;  // vctx_B == 0: no context set
    size_t vctx_bytes = 0;
    float* vscale = nullptr;
    std::vector<float> vscale_host;
    bool has_vace_context(int batch, int frames, int height, int width) const {
        return vctx_B == batch && vctx_F == frames && vctx_H == height && vctx_W == width;
    }
    int sst = -1, pe_w = -1, pe_b = -1, t1_w = -1, t1_b = -1, t2_w = -1, t2_b = -1, tp_w = -1, tp_b = -1, x1_w = -1, x1_b = -1, x2_w = -1,
        x2_b = -1, po_w = -1, po_b = -1;
    void *p_x1 = nullptr, *p_x2 = nullptr;  // text embedder weights, bf16
    // fg_wan_create_ex: the second time embedder `r_embedder` (Wan/network.py:615-619, 799-834) and what it is given
    // (time_cond_type "diff": t - r).  Both zero on a fg_wan_create handle.
    fg_wan_ext_config ext{0, 0};
    // fg_wan_create_i2v: the image-to-video network (WanI2V/network.py, Wan2.1-I2V convention).  The video (x_t, out, the samplers'
    // frames) then has i2v.latent_channels channels while the patch embedding reads cfg.in_channels = 2 latent + 4: vch() is the
    // video's count on every handle.  The condition (fg_wan_set_i2v_cond): the first-frame latents `ff` [B][latent][F][H][W] fp32, the
    // embedded image tokens `img_tok` [B * Li][D] bf16 and the blocks' kvi, all owned here and rewritten in place while their shapes
    // stay (the loops' graphs name them).
    bool is_i2v = false;
    fg_wan_i2v_config i2v{0, 0, 0};
    int vch() const { return is_i2v ? i2v.latent_channels : cfg.in_channels; }
    int in1_w = -1, in1_b = -1, if0_w = -1, if0_b = -1, if2_w = -1, if2_b = -1, in2_w = -1, in2_b = -1;  // condition_embedder.image_embedder
    void *p_if0 = nullptr, *p_if2 = nullptr;  // its two linears, bf16
    float* ff = nullptr;
    void* img_tok = nullptr;
    int ff_B = 0, ff_F = 0, ff_H = 0, ff_W = 0;  // ff_B == 0: no condition set
    int img_L = 0;                               // image tokens per sample of the condition (0: no image context)
    size_t ff_bytes = 0, img_rows = 0;           // what ff / img_tok + kvi are allocated for
    // fg_wan_create_ti2v: the Wan2.2-TI2V convention (WanI2V/network.py, concat_mask = False, expand_timesteps = True).  No extra
    // channels and no image keys; the condition (fg_wan_set_first_frame) is frame 0 of the first-frame latents, `ff0`
    // [B][latent][1][H][W] fp32, owned here and rewritten in place while its shape stays (the loops' graphs name it).  It feeds
    // frame 0's tokens, frame 0's embedder rows are zero and frame 0 of every result is its copy.
    bool is_ti2v = false;
    fg_wan_ti2v_config ti2v{0};
    float* ff0 = nullptr;
    int ff0_B = 0, ff0_H = 0, ff0_W = 0;  // ff0_B == 0: no condition set
    size_t ff0_bytes = 0;
    bool has_first_frame(int batch, int height, int width) const { return ff0_B == batch && ff0_H == height && ff0_W == width; }
    int r1_w = -1, r1_b = -1, r2_w = -1, r2_b = -1, rp_w = -1, rp_b = -1;
    float2 *tab_t = nullptr, *tab_h = nullptr, *tab_w = nullptr;  // RoPE axis tables
    int npt = 0, nph = 0, npw = 0;
    // fg_wan_sampler_run (engine_sampler.inc): the scalar ring and capture stream, and one graph per chunk of the loop (the chunk's
    // start frame, frame count and key length are baked in) in place of sampler.graph
    SamplerCache sampler;
    std::vector<GraphEntry> chunk_graphs;
    struct CacheState {
        int cache_B = 0, cache_cap = 0, text_B = 0, text_L = 0;
        size_t kv2_rows = 0;  // text rows (batch * text_len) the blocks' kv2 are allocated for; outlives clear_caches, which only zeroes text_B
        int stored_rows = 0;  // cache rows [0, stored_rows) hold K / V that a store_kv = 1 call wrote (the reference's per_tag["len"], network_causal.py:385-390)
    };
    // The reference keeps one cache sub-dict per cache_tag ("pos" / "neg", network_causal.py:331-412).  `cur` and the blocks'
    // kc / vc / kv2 are the SELECTED tag's set; the other tag's set waits here (fg_wan_select_cache_tag swaps them).  It is empty until
    // its tag is first selected and used: a handle that stays on tag 0 allocates nothing more.
    struct CacheSet {
        std::vector<void*> kc, vc, kv2;  // per block
        std::vector<void*> vkv2;         // per VACE block
        CacheState state;
    };
    CacheState cur;
    CacheSet other;
    int tag = 0;
    // f(state, kv, n) on the selected tag's set, then on the waiting one: kv(i) is block i's {kc, vc}, i < n
    template <typename F>
    int each_cache_set(F&& f) {
        if (int rc = f(cur, [&](size_t i) { return std::pair<void*, void*>(blocks[i].kc, blocks[i].vc); }, blocks.size())) return rc;
        return f(other.state, [&](size_t i) { return std::pair<void*, void*>(other.kc[i], other.vc[i]); }, other.kc.size());
    }
    // fg_wan_guided_sampler_run (engine_sampler.inc): its per-chunk graphs and the pinned host copy of the step scalars
    std::vector<GraphEntry> guided_graphs;
    GraphEntry full_guided_graph;  // fg_wan_full_guided_sampler_run: one graph for the video (fg_wan_full_sampler_run's is sampler.graph)
    double* pin = nullptr;
    size_t pin_doubles = 0;
    hipEvent_t pin_ev = nullptr;
    bool pin_used = false;
    // As in fg_dit: the GEMM weights are read from the caller's tensors at pack time only (into the bf16 copies p_qkv ...); every other
    // parameter is copied into `own` then, so that nothing points into the caller's memory between two packs (FSDP2 gathers one block,
    // packs it and frees it again: CausalWan.fully_shard).
    std::vector<float*> own;
    std::vector<char> pack_only, dirty;
    const float* P(int idx) const { return idx < 0 ? nullptr : (own[idx] ? own[idx] : params[idx].ptr); }
    bool is_logvar(int idx) const { return params[idx].name.find("logvar_linear") != std::string::npos; }
    // Before a buffer is freed: the graphs name every block's kc / vc / kv2 / kvi and the conditions, and their keys hold block 0's
    // addresses only, which the allocator may hand out again - no graph outlives a buffer it was captured on.
    void drop_graphs() {
        for (GraphEntry& g : chunk_graphs) g.drop();
        for (GraphEntry& g : guided_graphs) g.drop();
        full_guided_graph.drop();
        sampler.graph.drop();
    }
    // The one place a handle-owned buffer that the forward reads changes its address (wan_graph_key_tail names them): a buffer of the
    // wanted size stays where it is, and the graphs that name it stay valid; any other is freed behind the graphs and allocated anew
    // (want_bytes == 0: freed).  have_bytes is the buffer's own record - buffers that share one size field are given a copy of it each.
    int resize(void*& p, size_t& have_bytes, size_t want_bytes) {
        if (have_bytes == want_bytes) return FG_OK;
        drop_graphs();
        free(p);
        p = nullptr, have_bytes = 0;
        if (want_bytes == 0) return FG_OK;
        if (int rc = alloc(&p, want_bytes)) return rc;
        have_bytes = want_bytes;
        return FG_OK;
    }
};

namespace {

// What every entry point asks of a video: positive counts and whole 2 x 2 patches (a call without frames passes 1)
bool wan_shape_ok(int batch, int frames, int height, int width) {
    return batch > 0 && frames > 0 && height > 0 && width > 0 && !(height & 1) && !(width & 1);
}
// ... and of the bidirectional calls' token count: the kernels index rows with 32 bits
bool wan_rows_fit(int batch, int frames, int height, int width) {
    return (int64_t)batch * frames * (height / 2) * (width / 2) <= INT32_MAX / 2;
}

struct WanWs {
    float *tf, *th, *temb, *st, *tproj, *mod, *omod;
    float2* cs;
    void *x0, *x1, *y, *qkv, *qn, *att, *hid, *fa;
    void *kf, *vf;  // K / V of all frames in the block-causal (teacher-forcing) call: they stay out of the caches
    float* gs;  // split-K scratch of the token GEMMs (short grids: one sample's chunk)
    size_t gs_bytes;
    void *y8, *hid8;  // fp8 mode: the quantised A operands [M][D] (LayerNorm-modulate and attention outputs) / [M][ffn] (GELU hidden) ...
    float *ys, *hs;   // ... and their per-token scales [M]
    void *c0, *c1;    // VACE handle, bidirectional call: the control stream's ping-pong pair [M][D] bf16
};

size_t wan_plan(const fg_wan* h, int B, int Fr, int gh, int gw, Arena& A, WanWs& w, bool all_frames_kv = false) {
    const size_t D = h->D, BF = (size_t)B * Fr, M = BF * gh * gw, L = (size_t)Fr * gh * gw;
    w.tf = A.get<float>(BF * h->cfg.freq_dim);
    w.th = A.get<float>(BF * D);
    w.temb = A.get<float>(BF * D);
    w.st = A.get<float>(BF * D);
    w.tproj = A.get<float>(BF * 6 * D);
    w.mod = A.get<float>(BF * 6 * D);
    w.omod = A.get<float>(BF * 2 * D);
    w.cs = A.get<float2>(L * 64);
    w.x0 = A.take(M * D * 2);
    w.x1 = A.take(M * D * 2);
    w.y = A.take(M * D * 2);
    w.qkv = A.take(M * 3 * D * 2);
    w.qn = A.take(M * D * 2);
    w.att = A.take(M * D * 2);
    w.hid = A.take(M * (size_t)h->Fd * 2);
    w.fa = A.take(fa128_scratch_bytes(B, h->H, (int)L));
    w.gs_bytes = 4 * M * D * 4;  // up to 4 splits of an [M][D] output
    w.gs = (float*)A.take(w.gs_bytes);
    w.kf = w.vf = nullptr;
    if (Fr == h->cfg.total_num_frames || all_frames_kv) {  // (all_frames_kv: the bidirectional call, any frame count)
        w.kf = A.take(M * D * 2);
        w.vf = A.take(M * D * 2);
    }
    // (behind everything else, and nothing in the bf16 mode: that mode's plan and its size are what they were)
    w.y8 = A.take(h->fp8 ? M * D : 0);
    w.hid8 = A.take(h->fp8 ? M * (size_t)h->Fd : 0);
    w.ys = A.get<float>(h->fp8 ? M : 0);
    w.hs = A.get<float>(h->fp8 ? M : 0);
    // (VACE: the control stream's pair and nothing per hint - a hint is consumed by the GEMM that forms it.  The stream is seeded from
    // x0 before the first block overwrites it, so no copy of x0 is kept.)
    const bool vace = h->is_vace && all_frames_kv;
    w.c0 = A.take(vace ? M * D * 2 : 0);
    w.c1 = A.take(vace ? M * D * 2 : 0);
    return (A.off + 255) & ~(size_t)255;
}

// A block linear's input: bf16 tokens (scale == nullptr), or e4m3 bytes with their per-token scales (fp8 mode)
struct WanOperand {
    const void* p = nullptr;
    const float* scale = nullptr;
};

// The one linear dispatch: out = resid + gate * act(a W^T + bias).  An operand that carries scales runs on the e4m3 flavour of the
// token GEMM, W then being [N][K] e4m3fn bytes with the N channel scales behind them (wan_pack_linear); any other on the bf16 one.
int wan_gemm(WanOperand a, const void* w, const float* bias, void* out, int M, int N, int K, hipStream_t s, int act = 0, const float* gate = nullptr,
             int gate_stride = 0, int gate_rows = 1, const void* resid = nullptr, float* scratch = nullptr, size_t scratch_bytes = 0) {
    GemmArgs g;
    g.scratch = scratch; g.scratch_bytes = scratch_bytes;
    g.A = a.p; g.W = w; g.bias = bias; g.out = out; g.M = M; g.N = N; g.K = K; g.act = act;
    g.gate = gate; g.gate_stride = gate_stride; g.gate_rows = gate_rows; g.resid = resid;
    if (a.scale) {  // (no split-K in this flavour: the scratch goes unused)
        g.a_scale = a.scale;
        g.w_scale = reinterpret_cast<const float*>(static_cast<const char*>(w) + (size_t)N * K);
        if (!gemm_fp8_supported(g)) return fail(FG_EINVAL, "fp8 token GEMM %d x %d x %d unsupported (k %% 128, n %% 16)", M, N, K);
        HIP_TRY(launch_gemm_fp8(g, s));
        return FG_OK;
    }
    if (!gemm_bf16_supported(g)) return fail(FG_EINVAL, "token GEMM %d x %d x %d unsupported (k %% 64, n %% 16)", M, N, K);
    HIP_TRY(launch_gemm_bf16(g, s));
    return FG_OK;
}

// LayerNorm-modulate of the stream x as the mode's operand: y = LN(x) (1 + mod[scale_off ...]) + mod[shift_off ...], one modulation
// row per tpi tokens
int wan_modulate(const fg_wan* h, const void* x, const float* mod, int mstride, int shift_off, int scale_off, int M, int tpi, WanWs& w,
                 hipStream_t s, WanOperand& y) {
    if (h->fp8) {
        y = WanOperand{w.y8, w.ys};
        HIP_TRY(launch_dit_ln_modulate_fp8(h->D, x, mod, mstride, shift_off, scale_off, w.y8, w.ys, M, tpi, s));
    } else {
        y = WanOperand{w.y, nullptr};
        HIP_TRY(launch_dit_ln_modulate(1, h->D, x, mod, mstride, shift_off, scale_off, w.y, M, tpi, s));
    }
    return FG_OK;
}

// A bf16 token tensor [M][K] that a kernel left behind (an attention output, the GELU hidden) as the mode's operand: as it is, or
// quantised into q8 / scale (its rows cross the producing kernel's tiles, so the quantiser is a pass of its own, as in the DiT)
int wan_stage(const fg_wan* h, const void* src, int K, void* q8, float* scale, int M, hipStream_t s, WanOperand& a) {
    a = WanOperand{src, nullptr};
    if (h->fp8) {
        HIP_TRY(launch_quant_rows_fp8(1, src, q8, scale, M, K, s));
        a = WanOperand{q8, scale};
    }
    return FG_OK;
}

// A block linear's fp32 weight src [N][K] into rows [row0, row0 + N) of the packed [Ntot][K] matrix dst (the fused qkv weight takes
// three) in the mode's layout.  fp8: rows quantised on the device, the Ntot channel scales behind the Ntot K bytes.
int wan_pack_linear(const fg_wan* h, const float* src, void* dst, size_t row0, size_t Ntot, size_t N, size_t K, hipStream_t s) {
    if (h->fp8) {
        char* q = static_cast<char*>(dst);
        HIP_TRY(launch_quant_rows_fp8(0, src, q + row0 * K, reinterpret_cast<float*>(q + Ntot * K) + row0, (int64_t)N, (int)K, s));
    } else {
        HIP_TRY(launch_cvt_bf16(src, static_cast<__bf16*>(dst) + row0 * K, N * K, s));
    }
    return FG_OK;
}

// RoPE axis tables of WanRotaryPosEmbed: per axis [S][pairs] {cos, sin}, float64 angles (get_1d_rotary_pos_embed, theta 10000)
int wan_build_rope(fg_wan* h) {
    const int hd = h->cfg.head_dim, S = h->cfg.rope_max_seq_len;
    const int hdim = 2 * (hd / 6), tdim = hd - 2 * hdim;
    h->npt = tdim / 2, h->nph = hdim / 2, h->npw = hdim / 2;
    const int dims[3] = {tdim, hdim, hdim};
    float2** dst[3] = {&h->tab_t, &h->tab_h, &h->tab_w};
    for (int a = 0; a < 3; ++a) {
        const int np = dims[a] / 2;
        std::vector<float2> t((size_t)S * np);
        for (int p = 0; p < S; ++p)
            for (int i = 0; i < np; ++i) {
                const double f = 1.0 / pow(10000.0, (double)(2 * i) / (double)dims[a]);
                t[(size_t)p * np + i] = make_float2((float)cos((double)p * f), (float)sin((double)p * f));
            }
        int rc = h->alloc((void**)dst[a], t.size() * sizeof(float2));
        if (rc) return rc;
        HIP_TRY(hipMemcpy(*dst[a], t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice));
    }
    return FG_OK;
}

__global__ void wan_n2mod_kernel(const float* w, const float* b, float* mod, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < D) mod[i] = b[i], mod[D + i] = w[i] - 1.0f;
}
__global__ void wan_cat_kernel(const float* a, const float* b, const float* c, float* out, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < D) {
        out[i] = a[i];
        out[D + i] = b[i];
        if (c) out[2 * D + i] = c[i];
    }
}

// fg_wan_pack_group's part: device storage on the first call, then the bf16 GEMM weights and fused biases of the group
int wan_pack(fg_wan* h, const ParamGroup& in_group, hipStream_t s) {
    const size_t D = h->D, Fd = h->Fd, Td = h->cfg.text_dim;
    int rc;
    if (!h->device_ready) {
        if ((rc = h->alloc(&h->p_x1, D * Td * 2)) || (rc = h->alloc(&h->p_x2, D * D * 2))) return rc;
        const auto alloc_block = [&](fg_wan::Blk& b) -> int {
            if ((rc = h->alloc(&b.p_qkv, 3 * D * D * 2)) || (rc = h->alloc(&b.p_o, D * D * 2)) || (rc = h->alloc(&b.p_q2, D * D * 2)) ||
                (rc = h->alloc(&b.p_kv2, 2 * D * D * 2)) || (rc = h->alloc(&b.p_o2, D * D * 2)) || (rc = h->alloc(&b.p_f0, Fd * D * 2)) ||
                (rc = h->alloc(&b.p_f2, D * Fd * 2)) || (rc = h->alloc((void**)&b.b_qkv, 3 * D * 4)) ||
                (rc = h->alloc((void**)&b.b_kv2, 2 * D * 4)) || (rc = h->alloc((void**)&b.n2mod, 2 * D * 4)))
                return rc;
            if (h->i2v.image_dim > 0 && ((rc = h->alloc(&b.p_akv, 2 * D * D * 2)) || (rc = h->alloc((void**)&b.b_akv, 2 * D * 4)))) return rc;
            if (b.pin_w >= 0 && (rc = h->alloc(&b.p_pin, D * D * 2))) return rc;
            if (b.pout_w >= 0 && (rc = h->alloc(&b.p_pout, D * D * 2))) return rc;
            return FG_OK;
        };
        for (fg_wan::Blk& b : h->blocks)
            if ((rc = alloc_block(b))) return rc;
        for (fg_wan::Blk& b : h->vblocks)
            if ((rc = alloc_block(b))) return rc;
        if (h->is_vace) {
            const int n = h->vace.num_vace_layers;
            if ((rc = h->alloc((void**)&h->vscale, (size_t)n * D * 4))) return rc;
            WanVaceScales sc{};
            for (int j = 0; j < n; ++j) sc.v[j] = h->vscale_host[j];
            HIP_TRY(launch_wan_vace_scale_rows(sc, h->vscale, n, (int)D, s));
        }
        if (h->i2v.image_dim > 0) {
            const size_t Di = h->i2v.image_dim;
            if ((rc = h->alloc(&h->p_if0, Di * Di * 2)) || (rc = h->alloc(&h->p_if2, D * Di * 2))) return rc;
        }
        for (size_t i = 0; i < h->params.size(); ++i)
            if (!h->pack_only[i] && !h->is_logvar((int)i) && (rc = h->alloc((void**)&h->own[i], sizeof(float) * (size_t)h->params[i].numel))) return rc;
        if ((rc = wan_build_rope(h))) return rc;
        // (here, at pack time: never inside a sampler's graph capture; the text side runs the bf16 kernels in every mode)
        if (gemm_prepare(h->fp8 ? 1 | 4 : 1) != 0) return fail(FG_EHIP, "hipFuncSetAttribute(dynamic LDS) failed");
        h->device_ready = true;
    }
    auto raw = [&](int idx) { return h->params[idx].ptr; };
    if (in_group(h->params[h->x1_w].name)) {
        HIP_TRY(launch_cvt_bf16(raw(h->x1_w), h->p_x1, D * Td, s));
        HIP_TRY(launch_cvt_bf16(raw(h->x2_w), h->p_x2, D * D, s));
        if (h->i2v.image_dim > 0) {  // (the image embedder shares the text embedder's prefix: the same group)
            const size_t Di = h->i2v.image_dim;
            HIP_TRY(launch_cvt_bf16(raw(h->if0_w), h->p_if0, Di * Di, s));
            HIP_TRY(launch_cvt_bf16(raw(h->if2_w), h->p_if2, D * Di, s));
        }
    }
    const int g1 = (int)((D + 255) / 256);
    const auto pack_block = [&](fg_wan::Blk& b) -> int {
        const auto lin = [&](int idx, void* dst, size_t row0, size_t Ntot, size_t N, size_t K) {
            return wan_pack_linear(h, raw(idx), dst, row0, Ntot, N, K, s);
        };
        if ((rc = lin(b.q_w, b.p_qkv, 0, 3 * D, D, D)) || (rc = lin(b.k_w, b.p_qkv, D, 3 * D, D, D)) || (rc = lin(b.v_w, b.p_qkv, 2 * D, 3 * D, D, D)) ||
            (rc = lin(b.o_w, b.p_o, 0, D, D, D)) || (rc = lin(b.q2_w, b.p_q2, 0, D, D, D)) || (rc = lin(b.o2_w, b.p_o2, 0, D, D, D)) ||
            (rc = lin(b.f0_w, b.p_f0, 0, Fd, Fd, D)) || (rc = lin(b.f2_w, b.p_f2, 0, D, D, Fd)))
            return rc;
        __bf16* kv2 = (__bf16*)b.p_kv2;  // the text side: bf16 in every mode
        HIP_TRY(launch_cvt_bf16(raw(b.k2_w), kv2, D * D, s));
        HIP_TRY(launch_cvt_bf16(raw(b.v2_w), kv2 + D * D, D * D, s));
        hipLaunchKernelGGL(wan_cat_kernel, dim3(g1), dim3(256), 0, s, raw(b.q_b), raw(b.k_b), raw(b.v_b), b.b_qkv, (int)D);
        hipLaunchKernelGGL(wan_cat_kernel, dim3(g1), dim3(256), 0, s, raw(b.k2_b), raw(b.v2_b), (const float*)nullptr, b.b_kv2, (int)D);
        hipLaunchKernelGGL(wan_n2mod_kernel, dim3(g1), dim3(256), 0, s, raw(b.n2_w), raw(b.n2_b), b.n2mod, (int)D);
        if (b.p_akv) {  // the image side: bf16 in every mode, like the text side
            __bf16* akv = (__bf16*)b.p_akv;
            HIP_TRY(launch_cvt_bf16(raw(b.ak_w), akv, D * D, s));
            HIP_TRY(launch_cvt_bf16(raw(b.av_w), akv + D * D, D * D, s));
            hipLaunchKernelGGL(wan_cat_kernel, dim3(g1), dim3(256), 0, s, raw(b.ak_b), raw(b.av_b), (const float*)nullptr, b.b_akv, (int)D);
        }
        HIP_TRY(hipGetLastError());
        if (b.p_pin) HIP_TRY(launch_cvt_bf16(raw(b.pin_w), b.p_pin, D * D, s));  // (bf16 in every mode: see fastgen_amd.h)
        if (b.p_pout) HIP_TRY(launch_cvt_bf16(raw(b.pout_w), b.p_pout, D * D, s));
        return FG_OK;
    };
    for (fg_wan::Blk& b : h->blocks) {
        if (!in_group(h->params[b.q_w].name)) continue;  // (a block's parameters share their prefix: all of them in the group or none)
        if ((rc = pack_block(b))) return rc;
    }
    for (size_t k = 0; k < h->vblocks.size(); ++k) {
        // A VACE block's parameters arrive with the root group (the reference's fully_shard wraps `blocks` only), whose prefix says
        // nothing about them: the block is packed when ALL of its parameters are in the group - and bound, so that no null pointer is
        // read -, passed over when none is, and a group that holds some of them is refused.
        fg_wan::Blk& b = h->vblocks[k];
        int in = 0, total = 0, unbound = -1;
        b.each_param([&](int idx) {
            ++total;
            if (in_group(h->params[idx].name)) ++in;
            if (!h->params[idx].ptr) unbound = idx;
        });
        if (in == 0) continue;
        if (in != total) return fail(FG_ENOTREADY, "the group holds %d of the %d parameters of VACE block %d: a VACE block is packed whole", in, total, (int)k);
        if (unbound >= 0) return fail(FG_ENOTREADY, "parameter '%s' is not bound", h->params[unbound].name.c_str());
        if ((rc = pack_block(b))) return rc;
    }
    // the text caches (of both tags) were computed with the previous weights
    (void)h->each_cache_set([](fg_wan::CacheState& st, auto&&, size_t) {
        st.text_B = 0;
        return FG_OK;
    });
    h->ff_B = 0;                      // ... and so was the image-to-video condition
    h->vctx_B = 0;                    // ... and the VACE context (proj_in, vace_patch_embedding)
    return FG_OK;
}

// What fg_wan_create_ex / _i2v / _ti2v / _vace add to the plain network, each nullable
struct WanVariant {
    const fg_wan_ext_config* ext = nullptr;
    const fg_wan_i2v_config* i2v = nullptr;
    const fg_wan_ti2v_config* ti2v = nullptr;
    const fg_wan_vace_config* vace = nullptr;
};

// The five fg_wan_create* entry points: one table builder.  i2v == nullptr: the plain network's table (ti2v adds no parameter); vace:
// that table with the control branch's keys inserted.
int wan_create(const fg_wan_config* cfg, const WanVariant& var, fg_wan** out) {
    if (!cfg || !out) return fail(FG_EINVAL, "null argument");
    const auto [ext, i2v, ti2v, vace] = var;
    if (vace) {
        if (vace->vace_in_channels <= 0 || vace->vace_in_channels > 128)
            return fail(FG_EINVAL, "vace_in_channels %d outside (0, 128]", vace->vace_in_channels);
        if (vace->num_vace_layers < 1 || vace->num_vace_layers > 64) return fail(FG_EINVAL, "num_vace_layers %d outside [1, 64]", vace->num_vace_layers);
        for (int j = 0; j < vace->num_vace_layers; ++j)
            if (vace->vace_layers[j] < 0 || vace->vace_layers[j] >= cfg->num_layers || (j > 0 && vace->vace_layers[j] <= vace->vace_layers[j - 1]))
                return fail(FG_EINVAL, "vace_layers[%d] = %d: vace_layers must be strictly ascending in [0, num_layers = %d)", j, vace->vace_layers[j],
                            cfg->num_layers);
    }
    if (ti2v && (ti2v->latent_channels <= 0 || cfg->in_channels != ti2v->latent_channels || cfg->out_channels != ti2v->latent_channels))
        return fail(FG_EINVAL, "in_channels %d and out_channels %d must both equal latent_channels %d", cfg->in_channels, cfg->out_channels,
                    ti2v->latent_channels);
    if (i2v) {
        if (i2v->mask_channels != 4) return fail(FG_EINVAL, "mask_channels %d unsupported (4 = scale_factor_temporal)", i2v->mask_channels);
        if (i2v->latent_channels <= 0 || cfg->in_channels != 2 * i2v->latent_channels + i2v->mask_channels)
            return fail(FG_EINVAL, "in_channels %d must be 2 * latent_channels + mask_channels = %d", cfg->in_channels,
                        2 * i2v->latent_channels + i2v->mask_channels);
        if (cfg->out_channels != i2v->latent_channels)
            return fail(FG_EINVAL, "out_channels %d must equal latent_channels %d", cfg->out_channels, i2v->latent_channels);
        if (i2v->image_dim < 0 || (i2v->image_dim % 64)) return fail(FG_EINVAL, "image_dim %d must be 0 or a multiple of 64", i2v->image_dim);
    }
    const int Di = i2v ? i2v->image_dim : 0;
    if (ext && ((ext->r_timestep != 0 && ext->r_timestep != 1) || (ext->time_cond_diff != 0 && ext->time_cond_diff != 1)))
        return fail(FG_EINVAL, "r_timestep and time_cond_diff must be 0 or 1");
    if (cfg->head_dim != 128) return fail(FG_EINVAL, "head_dim %d unsupported (128)", cfg->head_dim);
    const int D = cfg->num_heads * cfg->head_dim;
    if (D != 256 && D != 384 && D != 1536 && D != 2048 && D != 3072 && D != 5120)
        return fail(FG_EINVAL, "inner dim %d unsupported (256, 384, 1536, 2048, 3072, 5120)", D);
    if (cfg->in_channels <= 0 || cfg->in_channels > 64 || cfg->out_channels <= 0 || cfg->out_channels > 64 || cfg->num_layers <= 0 ||
        (cfg->ffn_dim % 64) || (cfg->text_dim % 64) || cfg->freq_dim != 256 || cfg->rope_max_seq_len <= 0 || cfg->chunk_size <= 0 ||
        cfg->total_num_frames <= 0)
        return fail(FG_EINVAL, "bad channels / depth / ffn_dim / text_dim / freq_dim");
    if (cfg->compute_dtype != 0 && cfg->compute_dtype != FG_DTYPE_BF16 && cfg->compute_dtype != FG_DTYPE_FP8)
        return fail(FG_EINVAL, "compute_dtype %d unsupported (0 / FG_DTYPE_BF16, FG_DTYPE_FP8)", cfg->compute_dtype);
    const bool fp8 = cfg->compute_dtype == FG_DTYPE_FP8;
    if (fp8 && (cfg->ffn_dim % 128))  // (every supported inner dim is a multiple already)
        return fail(FG_EINVAL, "fp8 mode: ffn_dim %d must be a multiple of 128 (the K-step of the e4m3 MFMA)", cfg->ffn_dim);
    fg_wan* h = new fg_wan();
    h->fp8 = fp8;
    h->name_prefix = "transformer.";
    h->cfg = *cfg;
    h->D = D, h->Fd = cfg->ffn_dim, h->H = cfg->num_heads;
    const int C = cfg->in_channels, Fd = cfg->ffn_dim;
    // module order of diffusers' WanTransformer3DModel (a module's own parameters come before its submodules')
    h->sst = h->add("scale_shift_table", {1, 2, D});
    h->pe_w = h->add("patch_embedding.weight", {D, C, 1, 2});  // [D, C, 1, 2, 2] flattened to 4 dims: [D][C][1][4]
    h->params.back().ndim = 5;                                  // (reported as 5-d through fg_wan_param_info)
    h->params.back().numel = (int64_t)D * C * 4;
    h->pe_b = h->add("patch_embedding.bias", {D});
    if (vace) {  // (UNPINNED: the VACE keys and their places follow diffusers' module order as read, not a recorded list)
        h->vpe_w = h->add("vace_patch_embedding.weight", {D, vace->vace_in_channels, 1, 2});
        h->params.back().ndim = 5;
        h->params.back().numel = (int64_t)D * vace->vace_in_channels * 4;
        h->vpe_b = h->add("vace_patch_embedding.bias", {D});
    }
    h->t1_w = h->add("condition_embedder.time_embedder.linear_1.weight", {D, cfg->freq_dim});
    h->t1_b = h->add("condition_embedder.time_embedder.linear_1.bias", {D});
    h->t2_w = h->add("condition_embedder.time_embedder.linear_2.weight", {D, D});
    h->t2_b = h->add("condition_embedder.time_embedder.linear_2.bias", {D});
    h->tp_w = h->add("condition_embedder.time_proj.weight", {6 * D, D});
    h->tp_b = h->add("condition_embedder.time_proj.bias", {6 * D});
    h->x1_w = h->add("condition_embedder.text_embedder.linear_1.weight", {D, cfg->text_dim});
    h->x1_b = h->add("condition_embedder.text_embedder.linear_1.bias", {D});
    h->x2_w = h->add("condition_embedder.text_embedder.linear_2.weight", {D, D});
    h->x2_b = h->add("condition_embedder.text_embedder.linear_2.bias", {D});
    if (Di > 0) {
        // WanImageEmbedding (diffusers' WanTimeTextImageEmbedding.image_embedder, without pos_embed): norm1, ff, norm2.  UNPINNED: read
        // from the reference's key map (Wan/network.py:1029-1049) and diffusers' module order, not recorded from a run.
        const std::string ie = "condition_embedder.image_embedder.";
        h->in1_w = h->add(ie + "norm1.weight", {Di}); h->in1_b = h->add(ie + "norm1.bias", {Di});
        h->if0_w = h->add(ie + "ff.net.0.proj.weight", {Di, Di}); h->if0_b = h->add(ie + "ff.net.0.proj.bias", {Di});
        h->if2_w = h->add(ie + "ff.net.2.weight", {D, Di}); h->if2_b = h->add(ie + "ff.net.2.bias", {D});
        h->in2_w = h->add(ie + "norm2.weight", {D}); h->in2_b = h->add(ie + "norm2.bias", {D});
    }
    const int nvace = vace ? vace->num_vace_layers : 0;
    for (int i = 0; i < cfg->num_layers + nvace; ++i) {
        // (behind the main blocks the VACE blocks: scale_shift_table, proj_in (block 0 only), the main block's keys, proj_out)
        const bool vb = i >= cfg->num_layers;
        const std::string b = (vb ? "vace_blocks." + std::to_string(i - cfg->num_layers) : "blocks." + std::to_string(i)) + ".";
        fg_wan::Blk k;
        k.sst = h->add(b + "scale_shift_table", {1, 6, D});
        if (vb && i == cfg->num_layers) k.pin_w = h->add(b + "proj_in.weight", {D, D}), k.pin_b = h->add(b + "proj_in.bias", {D});
        k.q_w = h->add(b + "attn1.to_q.weight", {D, D}); k.q_b = h->add(b + "attn1.to_q.bias", {D});
        k.k_w = h->add(b + "attn1.to_k.weight", {D, D}); k.k_b = h->add(b + "attn1.to_k.bias", {D});
        k.v_w = h->add(b + "attn1.to_v.weight", {D, D}); k.v_b = h->add(b + "attn1.to_v.bias", {D});
        k.o_w = h->add(b + "attn1.to_out.0.weight", {D, D}); k.o_b = h->add(b + "attn1.to_out.0.bias", {D});
        k.nq = h->add(b + "attn1.norm_q.weight", {D}); k.nk = h->add(b + "attn1.norm_k.weight", {D});
        k.q2_w = h->add(b + "attn2.to_q.weight", {D, D}); k.q2_b = h->add(b + "attn2.to_q.bias", {D});
        k.k2_w = h->add(b + "attn2.to_k.weight", {D, D}); k.k2_b = h->add(b + "attn2.to_k.bias", {D});
        k.v2_w = h->add(b + "attn2.to_v.weight", {D, D}); k.v2_b = h->add(b + "attn2.to_v.bias", {D});
        k.o2_w = h->add(b + "attn2.to_out.0.weight", {D, D}); k.o2_b = h->add(b + "attn2.to_out.0.bias", {D});
        k.nq2 = h->add(b + "attn2.norm_q.weight", {D}); k.nk2 = h->add(b + "attn2.norm_k.weight", {D});
        if (Di > 0) {  // (UNPINNED, as the image embedder's keys above)
            k.ak_w = h->add(b + "attn2.add_k_proj.weight", {D, D}); k.ak_b = h->add(b + "attn2.add_k_proj.bias", {D});
            k.av_w = h->add(b + "attn2.add_v_proj.weight", {D, D}); k.av_b = h->add(b + "attn2.add_v_proj.bias", {D});
            k.nak = h->add(b + "attn2.norm_added_k.weight", {D});
        }
        k.n2_w = h->add(b + "norm2.weight", {D}); k.n2_b = h->add(b + "norm2.bias", {D});
        k.f0_w = h->add(b + "ffn.net.0.proj.weight", {Fd, D}); k.f0_b = h->add(b + "ffn.net.0.proj.bias", {Fd});
        k.f2_w = h->add(b + "ffn.net.2.weight", {D, Fd}); k.f2_b = h->add(b + "ffn.net.2.bias", {D});
        if (vb) k.pout_w = h->add(b + "proj_out.weight", {D, D}), k.pout_b = h->add(b + "proj_out.bias", {D});
        (vb ? h->vblocks : h->blocks).push_back(k);
    }
    h->po_w = h->add("proj_out.weight", {cfg->out_channels * 4, D});
    h->po_b = h->add("proj_out.bias", {cfg->out_channels * 4});
    h->add("logvar_linear.weight", {1, D});
    h->add("logvar_linear.bias", {1});
    if (ext) h->ext = *ext;
    if (h->ext.r_timestep) {
        // `init_embedder` (Wan/network.py:799-834): a deep copy of condition_embedder without its text_embedder, attached to the
        // transformer after logvar_linear.  (timesteps_proj and act_fn hold no parameters.)  Read from the code, not from a recorded list.
        h->r1_w = h->add("r_embedder.time_embedder.linear_1.weight", {D, cfg->freq_dim});
        h->r1_b = h->add("r_embedder.time_embedder.linear_1.bias", {D});
        h->r2_w = h->add("r_embedder.time_embedder.linear_2.weight", {D, D});
        h->r2_b = h->add("r_embedder.time_embedder.linear_2.bias", {D});
        h->rp_w = h->add("r_embedder.time_proj.weight", {6 * D, D});
        h->rp_b = h->add("r_embedder.time_proj.bias", {6 * D});
    }
    h->own.assign(h->params.size(), nullptr);
    h->pack_only.assign(h->params.size(), 0);
    h->dirty.assign(h->params.size(), 1);
    h->pack_only[h->x1_w] = h->pack_only[h->x2_w] = 1;
    for (const std::vector<fg_wan::Blk>* bl : {&h->blocks, &h->vblocks})
        for (const fg_wan::Blk& k : *bl)
            for (int idx : {k.q_w, k.k_w, k.v_w, k.o_w, k.q2_w, k.k2_w, k.v2_w, k.o2_w, k.f0_w, k.f2_w, k.ak_w, k.av_w, k.pin_w, k.pout_w})
                if (idx >= 0) h->pack_only[idx] = 1;
    if (Di > 0) h->pack_only[h->if0_w] = h->pack_only[h->if2_w] = 1;
    if (i2v) h->is_i2v = true, h->i2v = *i2v;
    if (ti2v) h->is_ti2v = true, h->ti2v = *ti2v;
    if (vace) {
        h->is_vace = true, h->vace = *vace;
        h->vscale_host.assign(nvace, 1.0f);  // (the reference's `new_ones(len(vace_layers))` when no scale is given, VaceWan/network.py:64-65)
    }
    *out = h;
    return FG_OK;
}
}  // namespace

extern "C" {

int fg_wan_create(const fg_wan_config* cfg, fg_wan** out) { return wan_create(cfg, {}, out); }
int fg_wan_create_ex(const fg_wan_config* cfg, const fg_wan_ext_config* ext, fg_wan** out) { return wan_create(cfg, {ext}, out); }
int fg_wan_create_i2v(const fg_wan_config* cfg, const fg_wan_ext_config* ext, const fg_wan_i2v_config* i2v, fg_wan** out) {
    if (!i2v) return fail(FG_EINVAL, "null argument");
    return wan_create(cfg, {ext, i2v}, out);
}

int fg_wan_create_ti2v(const fg_wan_config* cfg, const fg_wan_ext_config* ext, const fg_wan_ti2v_config* ti2v, fg_wan** out) {
    if (!ti2v) return fail(FG_EINVAL, "null argument");
    return wan_create(cfg, {ext, nullptr, ti2v}, out);
}

int fg_wan_create_vace(const fg_wan_config* cfg, const fg_wan_ext_config* ext, const fg_wan_vace_config* vace, fg_wan** out) {
    if (!vace) return fail(FG_EINVAL, "null argument");
    return wan_create(cfg, {ext, nullptr, nullptr, vace}, out);
}

int fg_wan_set_vace_scale(fg_wan* h, const float* scales_host, int n, void* stream) {
    if (!h || !scales_host) return fail(FG_EINVAL, "null argument");
    if (!h->is_vace) return fail(FG_EINVAL, "not a VACE handle (fg_wan_create_vace)");
    if (n != h->vace.num_vace_layers) return fail(FG_EINVAL, "%d scales for %d VACE layers", n, h->vace.num_vace_layers);
    for (int j = 0; j < n; ++j)
        if (!std::isfinite(scales_host[j])) return fail(FG_EINVAL, "scale %d is not finite", j);
    h->vscale_host.assign(scales_host, scales_host + n);
    if (h->vscale) {  // (before the first pack there are no rows yet: the pack writes them from vscale_host)
        WanVaceScales sc{};
        for (int j = 0; j < n; ++j) sc.v[j] = scales_host[j];
        HIP_TRY(launch_wan_vace_scale_rows(sc, h->vscale, n, h->D, (hipStream_t)stream));
    }
    return FG_OK;
}

int fg_wan_set_first_frame(fg_wan* h, const float* first_frame, int batch, int height, int width, void* stream) {
    if (!h || !first_frame) return fail(FG_EINVAL, "null argument");
    if (!h->is_ti2v) return fail(FG_EINVAL, "not a first-frame-replacement handle (fg_wan_create_ti2v)");
    if (!wan_shape_ok(batch, 1, height, width)) return fail(FG_EINVAL, "bad batch / size");
    const size_t bytes = (size_t)batch * h->ti2v.latent_channels * height * width * sizeof(float);
    h->ff0_B = 0;  // (nothing valid until the copy is enqueued)
    if (int rc = h->resize((void*&)h->ff0, h->ff0_bytes, bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(h->ff0, first_frame, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    h->ff0_B = batch, h->ff0_H = height, h->ff0_W = width;
    return FG_OK;
}

int fg_wan_first_frame_read(fg_wan* h, float* out, void* stream) {
    if (!h || !out) return fail(FG_EINVAL, "null argument");
    if (!h->is_ti2v) return fail(FG_EINVAL, "not a first-frame-replacement handle (fg_wan_create_ti2v)");
    if (h->ff0_B == 0) return fail(FG_ENOTREADY, "no first frame is set (call fg_wan_set_first_frame)");
    HIP_TRY(hipMemcpyAsync(out, h->ff0, h->ff0_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return FG_OK;
}

void fg_wan_destroy(fg_wan* h) {
    if (!h) return;
    h->drop_graphs();
    h->sampler.release();
    if (h->pin) (void)hipHostFree(h->pin);
    if (h->pin_ev) (void)hipEventDestroy(h->pin_ev);
    delete h;
}

int fg_wan_num_params(const fg_wan* h) { return h ? (int)h->params.size() : 0; }

int fg_wan_param_info(const fg_wan* h, int index, const char** name, int* ndim, int64_t shape[5]) {
    int nd = 0;
    const int rc = param_info(h, index, name, &nd, shape);
    if (rc) return rc;
    if (ndim) *ndim = nd;
    if (shape) {
        if (nd == 5) shape[2] = 1, shape[3] = 2, shape[4] = 2;  // the Conv3d patch embedding [D, C, 1, 2, 2]
        else shape[4] = 1;
    }
    return FG_OK;
}

int fg_wan_bind_param(fg_wan* h, const char* name, const float* device_ptr, int64_t numel) {
    int i;
    const int rc = bind_param(h, name, device_ptr, numel, &i);
    if (!rc) h->dirty[i] = 1;
    return rc;
}

int fg_wan_pack_weights(fg_wan* h, void* stream) { return fg_wan_pack_group(h, "", nullptr, stream); }

// Pack the parameters whose names start with `prefix` (and not with `exclude`, nullable): the unit FSDP2 gathers at a time
// ("transformer.blocks.7.", or "transformer." without "transformer.blocks." for the root group).
int fg_wan_pack_group(fg_wan* h, const char* prefix, const char* exclude, void* stream) {
    return pack_group(h, prefix, exclude, stream, wan_pack);
}

size_t fg_wan_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width) {
    if (!h || !wan_shape_ok(batch, frames, height, width)) return 0;
    Arena A;
    A.dry = true;
    WanWs w;
    const size_t chunk = wan_plan(h, batch, frames, height / 2, width / 2, A, w);
    // fg_wan_set_text's scratch: text bf16 [B * Lt][text_dim] + two [B * Lt][D] tensors (sized for Lt <= 1024)
    const size_t text = ((size_t)batch * 1024 * ((size_t)h->cfg.text_dim + 2 * (size_t)h->D) * 2 + 1024) & ~(size_t)255;
    return chunk > text ? chunk : text;
}

int fg_wan_clear_caches(fg_wan* h, void* stream) {
    if (!h) return fail(FG_EINVAL, "null handle");
    // the selected tag's set, and the same for the one that is not (the reference resets every tag's sub-dict)
    return h->each_cache_set([&](fg_wan::CacheState& st, auto&& kv, size_t n) -> int {
        const size_t bytes = (size_t)st.cache_B * st.cache_cap * h->D * 2;
        for (size_t i = 0; bytes > 0 && i < n; ++i) {
            HIP_TRY(hipMemsetAsync(kv(i).first, 0, bytes, (hipStream_t)stream));
            HIP_TRY(hipMemsetAsync(kv(i).second, 0, bytes, (hipStream_t)stream));
        }
        st.stored_rows = 0;
        st.text_B = 0;  // `is_init = False` of the cross-attention caches (network_causal.py:1046-1054)
        return FG_OK;
    });
}

int fg_wan_select_cache_tag(fg_wan* h, int tag) {
    if (!h) return fail(FG_EINVAL, "null handle");
    if (tag != 0 && tag != 1) return fail(FG_EINVAL, "cache tag %d: 0 (\"pos\") and 1 (\"neg\") are implemented", tag);
    if (tag == h->tag) return FG_OK;
    fg_wan::CacheSet& o = h->other;
    const size_t n = h->blocks.size();
    o.kc.resize(n, nullptr), o.vc.resize(n, nullptr), o.kv2.resize(n, nullptr);
    for (size_t i = 0; i < n; ++i) {
        std::swap(h->blocks[i].kc, o.kc[i]);
        std::swap(h->blocks[i].vc, o.vc[i]);
        std::swap(h->blocks[i].kv2, o.kv2[i]);
    }
    o.vkv2.resize(h->vblocks.size(), nullptr);
    for (size_t i = 0; i < h->vblocks.size(); ++i) std::swap(h->vblocks[i].kv2, o.vkv2[i]);
    std::swap(h->cur, o.state);
    h->tag = tag;
    return FG_OK;
}

int fg_wan_set_text(fg_wan* h, const float* text, int batch, int text_len, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !text || !workspace) return fail(FG_EINVAL, "null argument");
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_wan_pack_weights)");
    if (batch <= 0 || text_len <= 0 || text_len > 1024 || (((uintptr_t)workspace) & 255)) return fail(FG_EINVAL, "bad batch / text_len / workspace");
    hipStream_t s = (hipStream_t)stream;
    const size_t D = h->D, Td = h->cfg.text_dim, M = (size_t)batch * text_len;
    const size_t need = M * (Td + 2 * D) * 2 + 1024;
    if (need > workspace_bytes) return fail(FG_ENOMEM, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    char* ws = (char*)workspace;
    void* tb = ws;
    void* e1 = ws + ((M * Td * 2 + 255) & ~(size_t)255);
    void* e2 = (char*)e1 + ((M * D * 2 + 255) & ~(size_t)255);
    // (the sampler loops end with clear_caches, so every call sets its text again: the buffers stay where they are while their size
    // does, and the chunk graphs that name them stay valid)
    fg_wan::CacheState& st = h->cur;
    const size_t had = st.kv2_rows * 2 * D * 2;
    int rc;
    st.text_B = 0, st.kv2_rows = 0;  // (nothing valid until every block has its buffer and its keys)
    for (std::vector<fg_wan::Blk>* bl : {&h->blocks, &h->vblocks})  // (a VACE block has its own attn2.to_k / to_v / norm_k)
        for (fg_wan::Blk& b : *bl) {
            size_t have = had;
            if ((rc = h->resize(b.kv2, have, M * 2 * D * 2))) return rc;
        }
    st.kv2_rows = M;
    // text_embedder: Linear - GELU(tanh) - Linear (PixArtAlphaTextProjection); then per block k = norm_k(to_k(ctx)), v = to_v(ctx)
    HIP_TRY(launch_cvt_rows_bf16(text, tb, (int64_t)(M * Td), s));
    // (bf16 operands in every mode: this runs once per text)
    if ((rc = wan_gemm(WanOperand{tb}, h->p_x1, h->P(h->x1_b), e1, (int)M, (int)D, (int)Td, s, 1))) return rc;
    if ((rc = wan_gemm(WanOperand{e1}, h->p_x2, h->P(h->x2_b), e2, (int)M, (int)D, (int)D, s))) return rc;
    for (std::vector<fg_wan::Blk>* bl : {&h->blocks, &h->vblocks})
        for (fg_wan::Blk& b : *bl) {
            if ((rc = wan_gemm(WanOperand{e2}, b.p_kv2, b.b_kv2, b.kv2, (int)M, (int)(2 * D), (int)D, s))) return rc;
            HIP_TRY(launch_rms_rope((int)D, b.kv2, (int)(2 * D), h->P(b.nk2), h->cfg.eps, nullptr, b.kv2, (int64_t)text_len * 2 * D, 0, (int)(2 * D),
                                    (int)M, text_len, s));
        }
    st.text_B = batch, st.text_L = text_len;
    return FG_OK;
}

// fg_wan_set_i2v_cond's scratch for M = batch * image_len rows: LayerNorm'd image bf16 [M][Di], the hidden [M][Di], the embedder's
// output before norm2 [M][D], add_k | add_v [M][2 D]
size_t fg_wan_i2v_cond_workspace_bytes(const fg_wan* h, int batch, int image_len) {
    if (!h || !h->is_i2v || batch <= 0 || image_len < 0 || image_len > 1024) return 0;
    const size_t M = (size_t)batch * image_len, D = h->D, Di = h->i2v.image_dim;
    return ((M * (2 * Di + 3 * D) * 2 + 4 * 256) + 255) & ~(size_t)255;
}

int fg_wan_set_i2v_cond(fg_wan* h, const float* first_frame_cond, const float* image, int batch, int frames, int height, int width, int image_len,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !first_frame_cond) return fail(FG_EINVAL, "null argument");
    if (!h->is_i2v) return fail(FG_EINVAL, "not an image-to-video handle (fg_wan_create_i2v)");
    if (!wan_shape_ok(batch, frames, height, width)) return fail(FG_EINVAL, "bad batch / frames / size");
    if (image_len < 0 || image_len > 1024) return fail(FG_EINVAL, "image_len %d outside [0, 1024]", image_len);
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_wan_pack_weights)");
    hipStream_t s = (hipStream_t)stream;
    const size_t D = h->D, Di = h->i2v.image_dim;
    // image == NULL, image_len == 0 or no image parameters: the reference's empty image context (network_causal.py:297-302)
    const int Li = (image && Di > 0) ? image_len : 0, Lp = (Li + 31) & ~31;
    const size_t M = (size_t)batch * Li, rows = (size_t)batch * Lp;
    if (Li > 0) {
        const size_t need = fg_wan_i2v_cond_workspace_bytes(h, batch, Li);
        if (!workspace || (((uintptr_t)workspace) & 255)) return fail(FG_EINVAL, "bad workspace");
        if (need > workspace_bytes) return fail(FG_ENOMEM, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    }
    const size_t ff_bytes = (size_t)batch * h->i2v.latent_channels * frames * height * width * sizeof(float);
    int rc;
    h->ff_B = 0;  // (nothing valid until everything below is in place)
    if ((rc = h->resize((void*&)h->ff, h->ff_bytes, ff_bytes))) return rc;
    const size_t had = h->img_rows;
    h->img_rows = 0;
    size_t have = had * D * 2;
    if ((rc = h->resize(h->img_tok, have, rows * D * 2))) return rc;
    for (fg_wan::Blk& b : h->blocks) {  // whole 32-key tiles per sample, zero-filled: the padding rows stay zero
        have = had * 2 * D * 2;
        if ((rc = h->resize(b.kvi, have, rows * 2 * D * 2))) return rc;
        if (rows != had && rows > 0) HIP_TRY(hipMemsetAsync(b.kvi, 0, rows * 2 * D * 2, s));
    }
    h->img_rows = rows;
    HIP_TRY(hipMemcpyAsync(h->ff, first_frame_cond, ff_bytes, hipMemcpyDeviceToDevice, s));
    if (Li > 0) {
        auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
        char* ws = (char*)workspace;
        void* a0 = ws;
        void* a1 = (char*)a0 + up(M * Di * 2);
        void* a2 = (char*)a1 + up(M * Di * 2);
        void* a3 = (char*)a2 + up(M * D * 2);
        // WanImageEmbedding: FP32LayerNorm - Linear - GELU (erf) - Linear - FP32LayerNorm, eps 1e-5 (bf16 operands in every mode: once
        // per condition, like the text side)
        HIP_TRY(launch_wan_ln_rows(0, image, h->P(h->in1_w), h->P(h->in1_b), a0, (int)M, (int)Di, 1e-5f, s));
        if ((rc = wan_gemm(WanOperand{a0}, h->p_if0, h->P(h->if0_b), a1, (int)M, (int)Di, (int)Di, s))) return rc;
        HIP_TRY(launch_wan_gelu_erf(a1, (int64_t)(M * Di), s));
        if ((rc = wan_gemm(WanOperand{a1}, h->p_if2, h->P(h->if2_b), a2, (int)M, (int)D, (int)Di, s))) return rc;
        HIP_TRY(launch_wan_ln_rows(1, a2, h->P(h->in2_w), h->P(h->in2_b), h->img_tok, (int)M, (int)D, 1e-5f, s));
        // per block: k_img = norm_added_k(add_k_proj(img)), v_img = add_v_proj(img), scattered to the sample's padded rows
        for (fg_wan::Blk& b : h->blocks) {
            if ((rc = wan_gemm(WanOperand{h->img_tok}, b.p_akv, b.b_akv, a3, (int)M, (int)(2 * D), (int)D, s))) return rc;
            HIP_TRY(launch_rms_rope((int)D, a3, (int)(2 * D), h->P(b.nak), h->cfg.eps, nullptr, b.kvi, (int64_t)Lp * 2 * D, 0, (int)(2 * D), (int)M, Li, s));
            HIP_TRY(launch_rms_rope((int)D, (const __bf16*)a3 + D, (int)(2 * D), nullptr, h->cfg.eps, nullptr, (__bf16*)b.kvi + D, (int64_t)Lp * 2 * D, 0,
                                    (int)(2 * D), (int)M, Li, s));
        }
    }
    h->ff_B = batch, h->ff_F = frames, h->ff_H = height, h->ff_W = width, h->img_L = Li;
    return FG_OK;
}

int fg_wan_i2v_cond_read(fg_wan* h, int block, float* img_tokens, float* k_img, float* v_img, void* stream) {
    if (!h || !h->is_i2v) return fail(FG_EINVAL, "not an image-to-video handle (fg_wan_create_i2v)");
    if (block < 0 || block >= (int)h->blocks.size()) return fail(FG_EINVAL, "block %d outside [0, %d)", block, (int)h->blocks.size());
    if (h->ff_B == 0 || h->img_L == 0) return fail(FG_ENOTREADY, "no image context is set (call fg_wan_set_i2v_cond with image tokens)");
    hipStream_t s = (hipStream_t)stream;
    const int B = h->ff_B, Li = h->img_L, Lp = (Li + 31) & ~31, D = h->D;
    if (img_tokens) HIP_TRY(launch_from_act(1, h->img_tok, img_tokens, (int64_t)B * Li * D, s));
    if (!k_img && !v_img) return FG_OK;
    // the cache rows are strided [B][Lp][2 D]: a half (k or v) of the valid rows is gathered into a temporary contiguous bf16 tensor
    // (freed after the stream has drained: a test entry point, not a hot path)
    void* tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, (size_t)B * Li * D * 2));
    int rc = 0;
    for (int half = 0; half < 2 && !rc; ++half) {
        float* dst = half ? v_img : k_img;
        if (!dst) continue;
        for (int b = 0; b < B && !rc; ++b)
            rc = (int)hipMemcpy2DAsync((__bf16*)tmp + (size_t)b * Li * D, (size_t)D * 2,
                                       (const __bf16*)h->blocks[block].kvi + (size_t)b * Lp * 2 * D + half * D, (size_t)2 * D * 2, (size_t)D * 2,
                                       (size_t)Li, hipMemcpyDeviceToDevice, s);
        if (!rc) rc = launch_from_act(1, tmp, dst, (int64_t)B * Li * D, s);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(tmp);
    HIP_TRY((hipError_t)rc);
    return FG_OK;
}

// fg_wan_set_vace_context's scratch: the embedded context zero-padded to the video's token count, bf16 [B * L][D]
size_t fg_wan_vace_context_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width) {
    if (!h || !h->is_vace || !wan_shape_ok(batch, frames, height, width)) return 0;
    return ((size_t)batch * frames * (height / 2) * (width / 2) * h->D * 2 + 255) & ~(size_t)255;
}

int fg_wan_set_vace_context(fg_wan* h, const float* vid_context, int batch, int frames, int ctx_frames, int height, int width, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (!h || !vid_context) return fail(FG_EINVAL, "null argument");
    if (!h->is_vace) return fail(FG_EINVAL, "not a VACE handle (fg_wan_create_vace)");
    if (!wan_shape_ok(batch, frames, height, width)) return fail(FG_EINVAL, "bad batch / frames / size");
    if (ctx_frames <= 0 || ctx_frames > frames) return fail(FG_EINVAL, "ctx_frames %d outside [1, frames = %d]", ctx_frames, frames);
    if (!wan_rows_fit(batch, frames, height, width)) return fail(FG_EINVAL, "batch x tokens exceeds the kernels' 32-bit row index");
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_wan_pack_weights)");
    const size_t need = fg_wan_vace_context_workspace_bytes(h, batch, frames, height, width);
    if (!workspace || (((uintptr_t)workspace) & 255)) return fail(FG_EINVAL, "bad workspace");
    if (need > workspace_bytes) return fail(FG_ENOMEM, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const size_t D = h->D, L = (size_t)frames * (height / 2) * (width / 2), M = (size_t)batch * L;
    int rc;
    h->vctx_B = 0;  // (nothing valid until everything below is in place)
    if ((rc = h->resize(h->vctx, h->vctx_bytes, M * D * 2))) return rc;
    // `processed_control_states` (VaceWan/network.py:81-88): the embedded context's tokens, THEN zero rows up to the video's token
    // count; proj_in over all of them (a padded row becomes the bias).  bf16 operands in every mode: once per context, like the text.
    if (ctx_frames < frames) HIP_TRY(hipMemsetAsync(workspace, 0, M * D * 2, s));
    HIP_TRY(launch_wan_embed(WanEmbedSrc{vid_context, nullptr, WAN_EMBED_PLAIN, h->vace.vace_in_channels, ctx_frames, height, width}, h->P(h->vpe_w),
                             h->P(h->vpe_b), workspace, batch, (int)D, (int64_t)L, 0, s));
    const fg_wan::Blk& b0 = h->vblocks[0];
    if ((rc = wan_gemm(WanOperand{workspace}, b0.p_pin, h->P(b0.pin_b), h->vctx, (int)M, (int)D, (int)D, s))) return rc;
    h->vctx_B = batch, h->vctx_F = frames, h->vctx_H = height, h->vctx_W = width;
    return FG_OK;
}

int fg_wan_vace_context_read(fg_wan* h, float* ctx_in_out, void* stream) {
    if (!h || !ctx_in_out) return fail(FG_EINVAL, "null argument");
    if (!h->is_vace) return fail(FG_EINVAL, "not a VACE handle (fg_wan_create_vace)");
    if (h->vctx_B == 0) return fail(FG_ENOTREADY, "no VACE context is set (call fg_wan_set_vace_context)");
    HIP_TRY(launch_from_act(1, h->vctx, ctx_in_out, (int64_t)(h->vctx_bytes / 2), (hipStream_t)stream));
    return FG_OK;
}

namespace {
// where the handle's patch embedding reads its input: the virtual concat [x_t | mask | first_frame_cond] (image-to-video), x_t with
// frame 0's tokens from the first-frame condition (first-frame replacement), or x_t alone
WanEmbedSrc wan_embed_src(const fg_wan* h, const float* x_t, int frames, int height, int width) {
    if (h->is_i2v) return {x_t, h->ff, WAN_EMBED_CONCAT, h->i2v.latent_channels, frames, height, width};
    if (h->is_ti2v) return {x_t, h->ff0, WAN_EMBED_FRAME0, h->cfg.in_channels, frames, height, width};
    return {x_t, nullptr, WAN_EMBED_PLAIN, h->cfg.in_channels, frames, height, width};
}

// self-attention caches: [B][total_num_frames * frame_seqlen][D] per block, (re)allocated and zeroed when batch or frame size change
// (`_create_external_caches`, network_causal.py:708-812)
int wan_ensure_caches(fg_wan* h, int batch, int height, int width, hipStream_t s) {
    const int cap = h->cfg.total_num_frames * (height / 2) * (width / 2), D = h->D;
    fg_wan::CacheState& st = h->cur;
    if (st.cache_B == batch && st.cache_cap == cap) return FG_OK;
    const size_t had = (size_t)st.cache_B * st.cache_cap * D * 2, bytes = (size_t)batch * cap * D * 2;
    st.cache_B = st.cache_cap = 0;  // (nothing valid until every block has its new buffers)
    for (fg_wan::Blk& b : h->blocks) {
        size_t have_k = had, have_v = had;
        int rc;
        if ((rc = h->resize(b.kc, have_k, bytes)) || (rc = h->resize(b.vc, have_v, bytes))) return rc;
        HIP_TRY(hipMemsetAsync(b.kc, 0, bytes, s));
        HIP_TRY(hipMemsetAsync(b.vc, 0, bytes, s));
    }
    st.cache_B = batch, st.cache_cap = cap;
    st.stored_rows = 0;
    return FG_OK;
}

// FG_ENOTREADY unless the text and the handle's own condition are set for this call's shape.  batch: what the network is called with
// (a guided loop's stacked batch); hint: what the text, first-frame and VACE messages add to the setter's name ("", or the guided
// loops' " with [cond; neg_cond]" - the image-to-video message never carries it).
int wan_conditions_ready(const fg_wan* h, int batch, int frames, int height, int width, const char* hint = "") {
    if (h->cur.text_B != batch) return fail(FG_ENOTREADY, "no text condition for batch %d (call fg_wan_set_text%s)", batch, hint);
    if (h->is_i2v && (h->ff_B != batch || h->ff_F != frames || h->ff_H != height || h->ff_W != width))
        return fail(FG_ENOTREADY, "no image-to-video condition for batch %d, %d frames of %d x %d (call fg_wan_set_i2v_cond)", batch, frames, height, width);
    if (h->is_ti2v && !h->has_first_frame(batch, height, width))
        return fail(FG_ENOTREADY, "no first frame for batch %d of %d x %d (call fg_wan_set_first_frame%s)", batch, height, width, hint);
    if (h->is_vace && !h->has_vace_context(batch, frames, height, width))
        return fail(FG_ENOTREADY, "no VACE context for batch %d, %d frames of %d x %d (call fg_wan_set_vace_context%s)", batch, frames, height, width, hint);
    return FG_OK;
}

// What the handle is besides the plain network, as the refusals name it (nullptr: nothing): the bidirectional calls alone serve these
const char* wan_variant(const fg_wan* h) {
    if (h->is_i2v || h->is_ti2v) return "an image-to-video handle";
    return h->is_vace ? "a VACE handle" : nullptr;
}

// FG_EINVAL on such a handle; what: "calls" (wan_forward) or "loops" (the chunked samplers)
int wan_refuse_chunked(const fg_wan* h, const char* what) {
    if (const char* v = wan_variant(h)) return fail(FG_EINVAL, "the chunked / causal %s are not implemented for %s", what, v);
    return FG_OK;
}

// Everything handle-owned that a capture of wan_forward can bake in, behind the call's own arguments in the key of every Wan loop:
// the buffers' addresses (block 0's stand for every block's: they are resized together), the text's and image's lengths and the
// settings that choose a launch.  THE RULE: a new handle-owned buffer that wan_forward reads is added here and changes its address
// through fg_wan::resize alone - a key that misses it, or a free that does not drop the graphs, is a replay on freed memory.
void wan_graph_key_tail(const fg_wan* h, std::vector<int64_t>& key) {
    const fg_wan::Blk& b0 = h->blocks[0];
    const void* const bufs[] = {b0.kc, b0.kv2, b0.kvi, h->ff, h->ff0, h->vctx, h->vscale};
    for (const void* p : bufs) key.push_back((int64_t)(uintptr_t)p);
    key.insert(key.end(), {(int64_t)h->cur.text_L, (int64_t)h->img_L, (int64_t)h->fp8, (int64_t)h->ext.time_cond_diff});
}

// One time embedder on `rows` [BF]: Timesteps(256) -> Linear - SiLU - Linear into emb [BF][D], then time_proj(silu(emb)) into proj
// [BF][6 D] (w.tf, w.th and w.st are its scratch)
int wan_time_embedder(const fg_wan* h, const float* rows, int w1, int b1, int w2, int b2, int wp, int bp, float* emb, float* proj, int BF, WanWs& w,
                      hipStream_t s) {
    const int D = h->D, fq = h->cfg.freq_dim;
    HIP_TRY(launch_dit_fourier(rows, w.tf, BF, fq, s));
    HIP_TRY(launch_linear(w.tf, h->P(w1), h->P(b1), w.th, BF, fq, D, 1, s));
    HIP_TRY(launch_linear(w.th, h->P(w2), h->P(b2), emb, BF, D, D, 0, s));
    HIP_TRY(launch_silu(emb, w.st, (int64_t)BF * D, s));
    HIP_TRY(launch_linear(w.st, h->P(wp), h->P(bp), proj, BF, D, 6 * D, 0, s));
    return FG_OK;
}

// fg_wan_forward_features' taps (the parity tests): fp32 copies of the buffers the next kernel consumes, on the same stream
struct WanTaps {
    const int* blocks;
    const fg_wan_block_taps* taps;
    int n;
    float *tokens, *temb;
    float* tproj = nullptr;  // fg_wan_forward_full_features: timestep_proj [B * F][6 D] as the blocks read it (the r term added)
};

// The bidirectional call's additions (fg_wan_forward_full): the second embedder's rows and the blocks the call passes over
struct WanFull {
    const float* r_frames;
    const int* skip;
    int num_skip;
};

// What one bidirectional / chunked / block-causal call hands every block: the call's shapes, its workspace and where the keys live
struct WanBlockCall {
    WanWs& w;
    hipStream_t s;
    int batch, frames, fs, L, M, BF, block_causal, cache_start;
    int64_t cbs, MD;
    bool full;
};

// One transformer block on the token stream (x, xn) - the pair is swapped behind every residual GEMM, x is the stream on return.  The
// main blocks run it on the video tokens, the VACE blocks (fg_wan_create_vace) on the control stream: the same launches either way.
// bt (nullable): the block's taps.
int wan_block(fg_wan* h, fg_wan::Blk& b, void*& x, void*& xn, const fg_wan_block_taps* bt, const WanBlockCall& k) {
    const fg_wan_config& c = h->cfg;
    WanWs& w = k.w;
    hipStream_t s = k.s;
    const int D = h->D, batch = k.batch, frames = k.frames, fs = k.fs, L = k.L, M = k.M, BF = k.BF, block_causal = k.block_causal,
              cache_start = k.cache_start;
    const int64_t cbs = k.cbs, MD = k.MD;
    const bool full = k.full;
    int rc;
    HIP_TRY(launch_wan_mod(h->P(b.sst), w.tproj, w.mod, BF, 6, D, s));
    // 1. self-attention over the cached frames and this chunk.  K / V of the chunk go to their cache rows in every call (a call
    // with store_kv = 0 leaves rows that the chunk's store_kv = 1 call rewrites; the reference's cache length only moves there)
    WanOperand a;  // the operand the next linear reads
    if ((rc = wan_modulate(h, x, w.mod, 6 * D, 0, D, M, fs, w, s, a)) || (rc = wan_gemm(a, b.p_qkv, b.b_qkv, w.qkv, M, 3 * D, D, s))) return rc;
    const __bf16* qkv = (const __bf16*)w.qkv;
    HIP_TRY(launch_rms_rope(D, qkv, 3 * D, h->P(b.nq), c.eps, w.cs, w.qn, (int64_t)L * D, 0, D, M, L, s));
    if (block_causal) {
        // teacher / diffusion forcing over all frames (`_prepare_blockwise_causal_attn_mask`, network_causal.py:131-196): a query sees the
        // keys up to the end of its own chunk; the first chunk takes the remainder frames.  One attention launch per chunk over a
        // growing prefix of this call's K / V (the caches are the autoregressive calls' and stay untouched).
        HIP_TRY(launch_rms_rope(D, qkv + D, 3 * D, h->P(b.nk), c.eps, w.cs, w.kf, (int64_t)L * D, 0, D, M, L, s));
        HIP_TRY(launch_rms_rope(D, qkv + 2 * D, 3 * D, nullptr, c.eps, nullptr, w.vf, (int64_t)L * D, 0, D, M, L, s));
        const int chunk = full ? frames : c.chunk_size;  // (full attention: the one chunk sees every key)
        const int nch = frames / chunk, rem = frames % chunk;
        for (int ci = 0, f0 = 0; ci < (nch > 0 ? nch : 1); ++ci) {
            const int nf = nch == 0 ? rem : chunk + (ci == 0 ? rem : 0);
            const size_t q_off = (size_t)f0 * fs * D;
            HIP_TRY(launch_fa128((const __bf16*)w.qn + q_off, D, (int64_t)L * D, w.kf, w.vf, D, (int64_t)L * D, (__bf16*)w.att + q_off, D, (int64_t)L * D,
                                 batch, h->H, nf * fs, (f0 + nf) * fs, s, w.fa));
            f0 += nf;
        }
    } else {
        HIP_TRY(launch_rms_rope(D, qkv + D, 3 * D, h->P(b.nk), c.eps, w.cs, b.kc, cbs, cache_start, D, M, L, s));
        HIP_TRY(launch_rms_rope(D, qkv + 2 * D, 3 * D, nullptr, c.eps, nullptr, b.vc, cbs, cache_start, D, M, L, s));
        HIP_TRY(launch_fa128(w.qn, D, (int64_t)L * D, b.kc, b.vc, D, cbs, w.att, D, (int64_t)L * D, batch, h->H, L, cache_start + L, s, w.fa));
    }
    if (bt && bt->attn1) HIP_TRY(launch_from_act(1, w.att, bt->attn1, MD, s));
    if ((rc = wan_stage(h, w.att, D, w.y8, w.ys, M, s, a)) ||
        (rc = wan_gemm(a, b.p_o, h->P(b.o_b), xn, M, D, D, s, 0, w.mod + 2 * D, 6 * D, fs, x, w.gs, w.gs_bytes)))
        return rc;
    std::swap(x, xn);
    if (bt && bt->x_attn1) HIP_TRY(launch_from_act(1, x, bt->x_attn1, MD, s));
    // 2. cross-attention to the text
    if ((rc = wan_modulate(h, x, b.n2mod, 0, 0, D, M, M, w, s, a)) ||
        (rc = wan_gemm(a, b.p_q2, h->P(b.q2_b), w.qkv, M, D, D, s, 0, nullptr, 0, 1, nullptr, w.gs, w.gs_bytes)))
        return rc;
    HIP_TRY(launch_rms_rope(D, w.qkv, D, h->P(b.nq2), c.eps, nullptr, w.qn, (int64_t)L * D, 0, D, M, L, s));
    const int64_t tbs = (int64_t)h->cur.text_L * 2 * D;
    if (h->is_i2v && h->img_L > 0) {
        // ... and, separately normalised, to the image tokens; the two outputs summed (network_causal.py:294-358)
        const int64_t ibs = (int64_t)((h->img_L + 31) & ~31) * 2 * D;
        HIP_TRY(launch_wan_dual_xattn(w.qn, D, (int64_t)L * D, b.kv2, (const __bf16*)b.kv2 + D, 2 * D, tbs, h->cur.text_L, b.kvi, (const __bf16*)b.kvi + D,
                                      2 * D, ibs, h->img_L, w.att, D, (int64_t)L * D, batch, h->H, L, s));
    } else {
        HIP_TRY(launch_fa128(w.qn, D, (int64_t)L * D, b.kv2, (const __bf16*)b.kv2 + D, 2 * D, tbs, w.att, D, (int64_t)L * D, batch, h->H, L,
                             h->cur.text_L, s, w.fa));
    }
    if (bt && bt->attn2) HIP_TRY(launch_from_act(1, w.att, bt->attn2, MD, s));
    if ((rc = wan_stage(h, w.att, D, w.y8, w.ys, M, s, a)) ||
        (rc = wan_gemm(a, b.p_o2, h->P(b.o2_b), xn, M, D, D, s, 0, nullptr, 0, 1, x, w.gs, w.gs_bytes)))
        return rc;
    std::swap(x, xn);
    if (bt && bt->x_attn2) HIP_TRY(launch_from_act(1, x, bt->x_attn2, MD, s));
    // 3. feed-forward
    if ((rc = wan_modulate(h, x, w.mod, 6 * D, 3 * D, 4 * D, M, fs, w, s, a)) || (rc = wan_gemm(a, b.p_f0, h->P(b.f0_b), w.hid, M, h->Fd, D, s, 1)))
        return rc;
    if ((rc = wan_stage(h, w.hid, h->Fd, w.hid8, w.hs, M, s, a)) ||
        (rc = wan_gemm(a, b.p_f2, h->P(b.f2_b), xn, M, D, h->Fd, s, 0, w.mod + 5 * D, 6 * D, fs, x, w.gs, w.gs_bytes)))
        return rc;
    std::swap(x, xn);
    if (bt && bt->x_ffn) HIP_TRY(launch_from_act(1, x, bt->x_ffn, MD, s));
    return FG_OK;
}

bool wan_is_vace_layer(const fg_wan* h, int block) {
    for (int j = 0; j < h->vace.num_vace_layers; ++j)
        if (h->vace.vace_layers[j] == block) return true;
    return false;
}

// How many hints (= VACE blocks) a bidirectional call consumes: the VACE layers among the blocks it executes
int wan_vace_hints_consumed(const fg_wan* h, const WanFull* full) {
    if (!h->is_vace) return 0;
    int n = 0;
    for (int j = 0; j < h->vace.num_vace_layers; ++j) {
        bool skipped = false;
        for (int i = 0; full && i < full->num_skip; ++i) skipped |= full->skip[i] == h->vace.vace_layers[j];
        n += !skipped;
    }
    return n;
}

// block_causal: 0 - the autoregressive call on the caches; 1 - all total_num_frames frames under the block-wise causal mask; 2 - `full`
// given: all frames under full self-attention, the block-causal path with ONE chunk of `frames` frames (the same launches when
// chunk_size >= frames == total_num_frames), bounded by the RoPE table instead of total_num_frames
int wan_forward(fg_wan* h, const float* x_t, const float* t_frames, float* out, int batch, int frames, int height, int width,
                int cur_start_frame, int store_kv, int block_causal, void* workspace, size_t workspace_bytes, void* stream,
                const WanTaps* tp = nullptr, const WanFull* full = nullptr) {
    if (!h || !x_t || !t_frames || !out) return fail(FG_EINVAL, "null argument");
    if (full) {  // (what the arguments alone decide comes first, as in fg_wan_forward_features)
        if (full->r_frames && !h->ext.r_timestep) return fail(FG_EINVAL, "r_frames given, but the handle has no r_embedder (fg_wan_create_ex, r_timestep = 1)");
        if (full->num_skip < 0 || (full->num_skip > 0 && !full->skip)) return fail(FG_EINVAL, "bad skip_layers arguments");
        for (int i = 0; i < full->num_skip; ++i)
            if (full->skip[i] < 0 || full->skip[i] >= (int)h->blocks.size() || (i > 0 && full->skip[i] <= full->skip[i - 1]))
                return fail(FG_EINVAL, "skip_layers must be ascending block indices in [0, %d)", (int)h->blocks.size());
        if (frames > h->cfg.rope_max_seq_len)
            return fail(FG_EINVAL, "%d frames exceed the RoPE table (rope_max_seq_len = %d)", frames, h->cfg.rope_max_seq_len);
    }
    int rc;
    if (!full && (rc = wan_refuse_chunked(h, "calls"))) return rc;
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_wan_pack_weights)");
    if (!wan_shape_ok(batch, frames, height, width) || !workspace || (((uintptr_t)workspace) & 255))
        return fail(FG_EINVAL, "bad batch / frames / size / workspace");
    if ((rc = wan_conditions_ready(h, batch, frames, height, width))) return rc;
    if (tp)  // a VACE block that the call's skip_layers keep from running has nothing to tap
        for (int i = 0; i < tp->n; ++i)
            if (tp->blocks[i] >= (int)h->blocks.size() && tp->blocks[i] - (int)h->blocks.size() >= wan_vace_hints_consumed(h, full))
                return fail(FG_EINVAL, "VACE block %d is tapped but does not run under this call's skip_layers", tp->blocks[i] - (int)h->blocks.size());
    if (out == x_t) return fail(FG_EINVAL, "out must not alias x_t");
    hipStream_t s = (hipStream_t)stream;
    const fg_wan_config& c = h->cfg;
    const int D = h->D, gh = height / 2, gw = width / 2, fs = gh * gw, BF = batch * frames, L = frames * fs, M = batch * L;
    const int cap = c.total_num_frames * fs;
    if (full) {
        if (!wan_rows_fit(batch, frames, height, width)) return fail(FG_EINVAL, "batch x tokens exceeds the kernels' 32-bit row index");
    } else if (cur_start_frame < 0 || (cur_start_frame + frames) * fs > cap)
        return fail(FG_EINVAL, "frames [%d, %d) exceed the cache of total_num_frames = %d", cur_start_frame, cur_start_frame + frames, c.total_num_frames);
    if (fs > c.rope_max_seq_len * c.rope_max_seq_len || gh > c.rope_max_seq_len || gw > c.rope_max_seq_len) return fail(FG_EINVAL, "grid exceeds the RoPE table");
    Arena A;
    A.base = (char*)workspace;
    WanWs w;
    const size_t need = wan_plan(h, batch, frames, gh, gw, A, w, full != nullptr);
    if (need > workspace_bytes) return fail(FG_ENOMEM, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    if (block_causal && !full && frames != c.total_num_frames)
        return fail(FG_EINVAL, "the block-causal call takes all total_num_frames = %d frames, got %d", c.total_num_frames, frames);
    if (!block_causal && (rc = wan_ensure_caches(h, batch, height, width, s))) return rc;
    const int cache_start = cur_start_frame * fs;
    // The chunk's K / V go to their cache rows in EVERY call (attention then reads one contiguous prefix), where the reference writes
    // them only under store_kv and attends over [cache[:start] | current] (network_causal.py:385-400).  The two agree as long as a
    // store_kv = 0 call does not land on rows an earlier store_kv = 1 call filled - those are later chunks' context.  The student
    // loops (causvid.py:150-172, self_forcing.py:92-241) never do that; anything else is refused, not silently answered differently.
    if (!block_causal && !store_kv && cache_start < h->cur.stored_rows)
        return fail(FG_EINVAL, "store_kv = 0 at frame %d would overwrite cached keys / values (frames [0, %d) are stored): re-evaluating a stored "
                    "chunk without storing it is not implemented", cur_start_frame, h->cur.stored_rows / fs);
    // condition embedder, per frame (:586-590): Timesteps(256) -> Linear - SiLU - Linear; time_proj(silu(temb))
    const float* t_rows_in = t_frames;  // the caller's rows
    if (h->is_ti2v) {
        // expand_timesteps: the embedder sees mask * t per token (Wan/network.py:904-917) with the mask zero on latent frame 0 and
        // constant within a frame - the per-frame rows with frame 0's at zero (w.st: scratch until the SiLU below writes it)
        HIP_TRY(launch_wan_ti2v_zero_frame0(t_frames, w.st, BF, frames, s));
        t_frames = w.st;
    }
    if ((rc = wan_time_embedder(h, t_frames, h->t1_w, h->t1_b, h->t2_w, h->t2_b, h->tp_w, h->tp_b, w.temb, w.tproj, BF, w, s))) return rc;
    if (full && full->r_frames) {
        // r_embedder on r (or t - r), the `encoder_depth is None` branch (Wan/network.py:330-351): temb += remb, timestep_proj +=
        // r_timestep_proj.  Its scratch is the blocks' and the output layer's modulation rows, which nothing has written yet.
        float *rrow = w.mod, *remb = w.omod, *rproj = w.mod;
        // (first-frame replacement: the SiLU has rewritten the zeroed copy of t; the r rows are formed from the caller's values and their
        // frame 0 zeroed behind them - both masked rows are zero there, and so is their difference)
        HIP_TRY(launch_wan_r_rows(t_rows_in, full->r_frames, h->ext.time_cond_diff, rrow, BF, s));
        if (h->is_ti2v) HIP_TRY(launch_wan_ti2v_zero_frame0(rrow, rrow, BF, frames, s));
        if ((rc = wan_time_embedder(h, rrow, h->r1_w, h->r1_b, h->r2_w, h->r2_b, h->rp_w, h->rp_b, remb, rproj, BF, w, s))) return rc;
        HIP_TRY(launch_wan_add_r(w.temb, remb, (int64_t)BF * D, w.tproj, rproj, (int64_t)BF * 6 * D, s));
    }
    HIP_TRY(launch_wan_rope_table(h->tab_t, h->tab_h, h->tab_w, w.cs, L, fs, gw, cur_start_frame, c.rope_max_seq_len, h->npt, h->nph, h->npw, s));
    HIP_TRY(launch_wan_embed(wan_embed_src(h, x_t, frames, height, width), h->P(h->pe_w), h->P(h->pe_b), w.x0, batch, D, L, 0, s));
    void *x = w.x0, *xn = w.x1;
    const int64_t cbs = (int64_t)cap * D;
    const int64_t MD = (int64_t)M * D;
    if (tp && tp->temb) HIP_TRY(hipMemcpyAsync(tp->temb, w.temb, sizeof(float) * (size_t)BF * D, hipMemcpyDeviceToDevice, s));
    // (before the block loop: the r_embedder's scratch was w.mod, which the first launch_wan_mod rewrites from this very buffer)
    if (tp && tp->tproj) HIP_TRY(hipMemcpyAsync(tp->tproj, w.tproj, sizeof(float) * (size_t)BF * 6 * D, hipMemcpyDeviceToDevice, s));
    if (tp && tp->tokens) HIP_TRY(launch_from_act(1, x, tp->tokens, MD, s));
    const WanBlockCall call{w, s, batch, frames, fs, L, M, BF, block_causal, cache_start, cbs, MD, full != nullptr};
    // VACE: the control stream starts as c = proj_in(ctx) + x0 (ctx_in is the handle's, formed once per context), here, while x0 is
    // still whole.  vj: the hints consumed so far = the VACE blocks run so far.
    void *cx = w.c0, *cxn = w.c1;
    int vj = 0;
    if (h->is_vace) HIP_TRY(launch_wan_vace_seed(h->vctx, x, cx, MD, s));
    int ti = 0, blk_idx = 0, si = 0;
    for (fg_wan::Blk& b : h->blocks) {
        const fg_wan_block_taps* bt = (tp && ti < tp->n && tp->blocks[ti] == blk_idx) ? &tp->taps[ti++] : nullptr;
        const bool skip = full && si < full->num_skip && full->skip[si] == blk_idx;
        ++blk_idx;
        if (skip) {  // `if skip_layers is not None and idx in skip_layers: continue` (Wan/network.py:408)
            ++si;
            continue;
        }
        if ((rc = wan_block(h, b, x, xn, bt, call))) return rc;
        if (h->is_vace && wan_is_vace_layer(h, blk_idx - 1)) {
            // `hidden_states = hidden_states + control_hint * scale` with (hint, scale) popped from the FRONT of the list
            // (VaceWan/network.py:242-245): the j-th executed VACE layer takes hint j.  VACE block j depends on x0 and block j - 1 alone,
            // so it runs here, directly before its hint is consumed, and the hint proj_out_j(c) is the product of the GEMM that adds it:
            // x = x + scale_j * (c Wout^T + b), rounded once.  A hint that no executed layer consumes is never computed.
            fg_wan::Blk& vb = h->vblocks[vj];
            const fg_wan_block_taps* vt = nullptr;
            for (int i = 0; tp && i < tp->n; ++i)
                if (tp->blocks[i] == (int)h->blocks.size() + vj) vt = &tp->taps[i];
            if ((rc = wan_block(h, vb, cx, cxn, vt, call)) ||
                (rc = wan_gemm(WanOperand{cx}, vb.p_pout, h->P(vb.pout_b), xn, M, D, D, s, 0, h->vscale + (size_t)vj * D, D, M, x, w.gs, w.gs_bytes)))
                return rc;
            std::swap(x, xn);
            ++vj;
        }
    }
    if (!block_causal && store_kv && cache_start + L > h->cur.stored_rows) h->cur.stored_rows = cache_start + L;
    HIP_TRY(launch_wan_outmod(h->P(h->sst), w.temb, w.omod, BF, D, s));
    HIP_TRY(launch_wan_ti2v_final(D, x, w.omod, h->P(h->po_w), h->P(h->po_b), h->is_ti2v ? h->ff0 : nullptr, out, M, frames, gh, gw, c.out_channels,
                                  c.eps, 0, s));
    return FG_OK;
}
}  // namespace

int fg_wan_forward(fg_wan* h, const float* x_t, const float* t_frames, float* out, int batch, int frames, int height, int width,
                   int cur_start_frame, int store_kv, void* workspace, size_t workspace_bytes, void* stream) {
    return wan_forward(h, x_t, t_frames, out, batch, frames, height, width, cur_start_frame, store_kv, 0, workspace, workspace_bytes, stream);
}

int fg_wan_forward_block_causal(fg_wan* h, const float* x_t, const float* t_frames, float* out, int batch, int frames, int height, int width,
                                void* workspace, size_t workspace_bytes, void* stream) {
    return wan_forward(h, x_t, t_frames, out, batch, frames, height, width, 0, 0, 1, workspace, workspace_bytes, stream);
}

namespace {
int wan_check_taps(const fg_wan* h, const int* tap_blocks, const fg_wan_block_taps* taps, int num_taps) {
    if (!h) return fail(FG_EINVAL, "null argument");
    if (num_taps < 0 || (num_taps > 0 && (!tap_blocks || !taps))) return fail(FG_EINVAL, "bad tap arguments");
    for (int i = 0; i < num_taps; ++i)
        if (tap_blocks[i] < 0 || tap_blocks[i] >= (int)(h->blocks.size() + h->vblocks.size()) || (i > 0 && tap_blocks[i] <= tap_blocks[i - 1]))
            return fail(FG_EINVAL, "tap_blocks must be ascending block indices in [0, %d)", (int)(h->blocks.size() + h->vblocks.size()));
    return FG_OK;
}
}  // namespace

int fg_wan_forward_features(fg_wan* h, const float* x_t, const float* t_frames, float* out, int batch, int frames, int height, int width,
                            int cur_start_frame, int store_kv, int block_causal, const int* tap_blocks, const fg_wan_block_taps* taps,
                            int num_taps, float* tokens_out, float* temb_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = wan_check_taps(h, tap_blocks, taps, num_taps)) return rc;
    if (block_causal && (cur_start_frame != 0 || store_kv)) return fail(FG_EINVAL, "the block-causal call starts at frame 0 and stores nothing");
    const WanTaps tp{tap_blocks, taps, num_taps, tokens_out, temb_out};
    return wan_forward(h, x_t, t_frames, out, batch, frames, height, width, cur_start_frame, store_kv, block_causal ? 1 : 0, workspace,
                       workspace_bytes, stream, &tp);
}

size_t fg_wan_full_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width) {
    if (!h || !wan_shape_ok(batch, frames, height, width)) return 0;
    Arena A;
    A.dry = true;
    WanWs w;
    const size_t net = wan_plan(h, batch, frames, height / 2, width / 2, A, w, true);
    const size_t text = fg_wan_workspace_bytes(h, batch, 1, 2, 2);  // (at least fg_wan_set_text's scratch)
    return net > text ? net : text;
}

int fg_wan_forward_full(fg_wan* h, const float* x_t, const float* t_frames, const float* r_frames, float* out, int batch, int frames, int height,
                        int width, const int* skip_layers, int num_skip, void* workspace, size_t workspace_bytes, void* stream) {
    const WanFull full{r_frames, skip_layers, num_skip};
    return wan_forward(h, x_t, t_frames, out, batch, frames, height, width, 0, 0, 2, workspace, workspace_bytes, stream, nullptr, &full);
}

int fg_wan_forward_full_features(fg_wan* h, const float* x_t, const float* t_frames, const float* r_frames, float* out, int batch, int frames,
                                 int height, int width, const int* skip_layers, int num_skip, const int* tap_blocks,
                                 const fg_wan_block_taps* taps, int num_taps, float* tokens_out, float* temb_out, float* tproj_out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = wan_check_taps(h, tap_blocks, taps, num_taps)) return rc;
    // a skipped block runs no kernel: it has nothing to tap (wan_forward checks the skip list itself)
    if (num_skip > 0 && skip_layers)
        for (int i = 0; i < num_taps; ++i)
            for (int j = 0; j < num_skip; ++j)
                if (tap_blocks[i] == skip_layers[j]) return fail(FG_EINVAL, "block %d is both tapped and in skip_layers", tap_blocks[i]);
    WanTaps tp{tap_blocks, taps, num_taps, tokens_out, temb_out};
    tp.tproj = tproj_out;
    const WanFull full{r_frames, skip_layers, num_skip};
    return wan_forward(h, x_t, t_frames, out, batch, frames, height, width, 0, 0, 2, workspace, workspace_bytes, stream, &tp, &full);
}
