// EDM2 U-Net engine (EDM2Precond, reference fastgen/networks/EDM2/network.py): module layout and state-dict order, weight normalisation
// and packing with the magnitude-preserving constants folded in, workspace plan, the forward schedule, the per-block entry points and
// the x0 sampler loop.  Textually included by engine.hip inside its `extern "C"` region (the handle is a HandleBase; setup_ws, the
// SamplerCache and the student loop are engine.hip's).  Convolutions and attention are adm.hip's kernels; the rest is edm2.hip.  Forward only, split-bf16 and bf16 convolutions, fp32 activations.
}  // extern "C" (reopened below)

namespace {

struct E2Block {
    std::string key;
    bool enc = true, up = false, down = false, attn = false;
    int cin = 0, cout = 0, res_in = 0, res_out = 0;
    int skip_c = 0;  // decoder: channels of the popped skip (mp_cat's second operand), else 0
    int off = 0;     // first row of this block's emb_linear in the stacked modulation matrix
    int gain = -1, res0 = -1, lin = -1, res1 = -1, skip = -1, qkv = -1, proj = -1;
    void *p_res0 = nullptr, *p_res1 = nullptr, *p_skip = nullptr, *p_qkv = nullptr, *p_proj = nullptr;
    float2* cat_ab = nullptr;  // decoder with a skip: [cin] {wa | wb, 0}, mp_cat's weights in conv_res0's prologue
    float wa = 1.f, wb = 1.f;
};

struct E2Ws {
    float *coef, *four, *e, *lab, *emb, *cc;
    float2* ab_all;  // [B][total] conv_res1 prologue rows of every block
    float* stem_in;
    std::vector<float*> skip;
    float *xa, *xb, *h, *s, *t1, *qkv, *a, *F;
    float *x, *x_pred, *eps;
    double* tl;
    uint64_t* seed;
};

constexpr int kE2StemPad = 32;  // stem operand channels: [c_in x | 1 | zeros] padded to one K-chunk of the conv

double mp_sum_norm(double t) { return std::sqrt((1 - t) * (1 - t) + t * t); }

}  // namespace

struct fg_edm2 : HandleBase {
    fg_edm2_config cfg;
    int cmode = 0;
    int cnoise = 0, cemb = 0, total = 0, stem_c = 0, out_cin = 0;
    std::vector<E2Block> enc, dec;
    std::vector<int> skip_c, skip_res;
    int out_gain = -1, freqs = -1, phases = -1, emb_noise = -1, emb_label = -1, stem_w = -1, out_w = -1;
    bool training = false;
    // owned device memory
    float *w_noise = nullptr, *w_label = nullptr, *w_mod = nullptr, *scratch = nullptr;
    float2* ones = nullptr;  // [max width] {1, 0}: conv_res0's plain silu(x) prologue
    void *p_stem = nullptr, *p_out = nullptr;
    size_t scratch_elems = 0;
    int max_c = 0;
    SamplerCache sampler;  // fg_edm2_sampler_run

    double shift() const { return training ? 0.0 : cfg.sigma_shift; }
    const float* P(int idx) const { return idx >= 0 ? params[idx].ptr : nullptr; }
};

namespace {

// EMD2UNet.__init__: the module order of the reference, so param_info lists the state_dict() order.
void e2_build_layout(fg_edm2* h) {
    const fg_edm2_config& c = h->cfg;
    const int mc = c.model_channels;
    std::vector<int> cblock(c.num_levels);
    int cmax = 0;
    for (int l = 0; l < c.num_levels; ++l) cblock[l] = mc * c.channel_mult[l], cmax = std::max(cmax, cblock[l]);
    h->cnoise = c.channel_mult_noise > 0 ? mc * c.channel_mult_noise : cblock[0];
    h->cemb = c.channel_mult_emb > 0 ? mc * c.channel_mult_emb : cmax;
    const int E = h->cemb;
    h->out_gain = h->add("unet.out_gain", {1});
    h->freqs = h->add("unet.emb_fourier.freqs", {h->cnoise});
    h->phases = h->add("unet.emb_fourier.phases", {h->cnoise});
    h->emb_noise = h->add("unet.emb_noise.weight", {E, h->cnoise});
    if (c.label_dim) h->emb_label = h->add("unet.emb_label.weight", {E, c.label_dim});
    auto attn_at = [&](int res) {
        for (int i = 0; i < c.num_attn_resolutions; ++i)
            if (c.attn_resolutions[i] == res) return true;
        return false;
    };
    auto block = [&](const std::string& key, bool enc, int cin, int cout, int res_out, bool up, bool down, bool attn) {
        E2Block b;
        b.key = key, b.enc = enc, b.cin = cin, b.cout = cout, b.res_out = res_out, b.up = up, b.down = down, b.attn = attn;
        b.res_in = down ? 2 * res_out : up ? res_out / 2 : res_out;
        const std::string p = key + ".";
        b.gain = h->add(p + "emb_gain", {1});
        b.res0 = h->add(p + "conv_res0.weight", {cout, enc ? cout : cin, 3, 3});
        b.lin = h->add(p + "emb_linear.weight", {cout, E});
        b.res1 = h->add(p + "conv_res1.weight", {cout, cout, 3, 3});
        if (cin != cout) b.skip = h->add(p + "conv_skip.weight", {cout, cin, 1, 1});
        if (attn) {
            b.qkv = h->add(p + "attn_qkv.weight", {3 * cout, cout, 1, 1});
            b.proj = h->add(p + "attn_proj.weight", {cout, cout, 1, 1});
        }
        b.off = h->total;
        h->total += cout;
        h->max_c = std::max(h->max_c, std::max(cin, cout));
        return b;
    };
    auto rn = [](int r) { return std::to_string(r) + "x" + std::to_string(r); };
    int cout = c.img_channels + 1;
    for (int level = 0; level < c.num_levels; ++level) {
        const int res = c.img_resolution >> level;
        const std::string r = "unet.enc." + rn(res);
        if (level == 0) {
            h->stem_c = cblock[0];
            h->stem_w = h->add(r + "_conv.weight", {h->stem_c, cout, 3, 3});
            cout = h->stem_c;
        } else {
            h->enc.push_back(block(r + "_down", true, cout, cout, res, false, true, false));
        }
        h->skip_c.push_back(cout), h->skip_res.push_back(res);
        for (int i = 0; i < c.num_blocks; ++i) {
            const int cin = cout;
            cout = cblock[level];
            h->enc.push_back(block(r + "_block" + std::to_string(i), true, cin, cout, res, false, false, attn_at(res)));
            h->skip_c.push_back(cout), h->skip_res.push_back(res);
        }
    }
    std::vector<int> skips = h->skip_c;
    for (int level = c.num_levels - 1; level >= 0; --level) {
        const int res = c.img_resolution >> level;
        const std::string r = "unet.dec." + rn(res);
        if (level == c.num_levels - 1) {
            h->dec.push_back(block(r + "_in0", false, cout, cout, res, false, false, true));
            h->dec.push_back(block(r + "_in1", false, cout, cout, res, false, false, false));
        } else {
            h->dec.push_back(block(r + "_up", false, cout, cout, res, true, false, false));
        }
        for (int i = 0; i <= c.num_blocks; ++i) {
            const int sc = skips.back();
            skips.pop_back();
            const int cin = cout + sc;
            cout = cblock[level];
            E2Block b = block(r + "_block" + std::to_string(i), false, cin, cout, res, false, false, attn_at(res));
            b.skip_c = sc;
            // mp_cat(x, skip, t = concat_balance): wa = C / sqrt(Na) (1 - t), wb = C / sqrt(Nb) t, C = sqrt((Na + Nb) / ((1-t)^2 + t^2))
            const double t = c.concat_balance, na = cin - sc, nb = sc;
            const double C = std::sqrt((na + nb) / ((1 - t) * (1 - t) + t * t));
            b.wa = (float)(C / std::sqrt(na) * (1 - t));
            b.wb = (float)(C / std::sqrt(nb) * t);
            h->dec.push_back(b);
        }
    }
    h->out_cin = cout;
    h->out_w = h->add("unet.out_conv.weight", {c.img_channels, cout, 3, 3});
}

int e2_check_supported(const fg_edm2* h) {
    const fg_edm2_config& c = h->cfg;
    const int R = c.img_resolution;
    if (R > 64 || R < 8 || (R & (R - 1))) return fail(FG_EINVAL, "EDM2: img_resolution %d unsupported (8 .. 64, power of two)", R);
    if ((R >> (c.num_levels - 1)) < 8) return fail(FG_EINVAL, "EDM2: lowest resolution %d < 8 unsupported", R >> (c.num_levels - 1));
    if (c.img_channels < 1 || c.img_channels > 4) return fail(FG_EINVAL, "EDM2: img_channels %d unsupported (1 .. 4)", c.img_channels);
    for (int i = 0; i < c.num_levels; ++i)
        if ((c.model_channels * c.channel_mult[i]) % 64)
            return fail(FG_EINVAL, "EDM2: level %d has %d channels, not a multiple of 64", i, c.model_channels * c.channel_mult[i]);
    if (h->cnoise <= 0 || h->cemb <= 0) return fail(FG_EINVAL, "EDM2: bad embedding widths");
    for (const auto* list : {&h->enc, &h->dec})
        for (const E2Block& b : *list)
            if (b.attn && (b.res_out < 8 || (b.res_out * b.res_out) % 64))
                return fail(FG_EINVAL, "%s: attention at %dx%d unsupported (resolution >= 8)", b.key.c_str(), b.res_out, b.res_out);
    return FG_OK;
}

size_t e2_plan(const fg_edm2* h, int B, Arena& A, E2Ws& w) {
    const fg_edm2_config& c = h->cfg;
    size_t max_act = 0, max_attn = 1;
    for (const auto* list : {&h->enc, &h->dec})
        for (const E2Block& b : *list) {
            const size_t hw = (size_t)b.res_out * b.res_out;
            max_act = std::max(max_act, hw * b.cout);
            if (b.attn) max_attn = std::max(max_attn, hw * b.cout);
        }
    const int R = c.img_resolution;
    w.coef = A.get<float>(5 * (size_t)B);
    w.four = A.get<float>((size_t)B * h->cnoise);
    w.e = A.get<float>((size_t)B * h->cemb);
    w.lab = A.get<float>((size_t)B * h->cemb);
    w.emb = A.get<float>((size_t)B * h->cemb);
    w.cc = A.get<float>((size_t)B * h->total);
    w.ab_all = A.get<float2>((size_t)B * h->total);
    w.stem_in = A.get<float>((size_t)B * R * R * kE2StemPad);
    w.skip.clear();
    for (size_t i = 0; i < h->skip_c.size(); ++i) w.skip.push_back(A.get<float>((size_t)B * h->skip_res[i] * h->skip_res[i] * h->skip_c[i]));
    w.xa = A.get<float>((size_t)B * max_act);
    w.xb = A.get<float>((size_t)B * max_act);
    w.h = A.get<float>((size_t)B * max_act);
    w.s = A.get<float>((size_t)B * max_act);
    w.t1 = A.get<float>((size_t)B * max_attn);
    w.qkv = A.get<float>((size_t)B * 3 * max_attn);
    w.a = A.get<float>((size_t)B * max_attn);
    const size_t img = (size_t)B * c.img_channels * R * R;
    w.F = A.get<float>(img);
    w.x = A.get<float>(img);
    w.x_pred = A.get<float>(img);
    w.eps = A.get<float>(img);
    w.tl = A.get<double>(ScalarRing::kDoubles);
    w.seed = A.get<uint64_t>(8);
    return (A.off + 255) & ~(size_t)255;
}

// normalize + MP scaling (+ folds) of one conv's weights into the scratch copy, then the ADM conv packing
int e2_pack_conv(fg_edm2* h, void** dst, int widx, int cout, int cin, int cin_pad, int ks, const float* gain, float e0, float e1, int c_split,
                 hipStream_t s) {
    int rc;
    if (!*dst && (rc = h->alloc(dst, adm_conv_pack_elems(h->cmode, cout, cin_pad, ks) * sizeof(__bf16)))) return rc;
    HIP_TRY(edm2_launch_prep_weight(h->P(widx), h->scratch, cout, cin, cin_pad, ks * ks, gain, e0, e1, c_split, s));
    HIP_TRY(adm_pack_conv_weights(h->cmode, h->scratch, *dst, cout, cin_pad, ks, s));
    return FG_OK;
}

int e2_pack(fg_edm2* h, hipStream_t s) {
    const fg_edm2_config& c = h->cfg;
    int rc;
    if (!h->device_ready) {
        size_t sc = (size_t)h->stem_c * kE2StemPad * 9;
        for (const auto* list : {&h->enc, &h->dec})
            for (const E2Block& b : *list) sc = std::max(sc, (size_t)b.cout * std::max(b.cin, b.cout) * 9 + (size_t)3 * b.cout * b.cout);
        h->scratch_elems = sc;
        if ((rc = h->alloc((void**)&h->scratch, sizeof(float) * sc))) return rc;
        if ((rc = h->alloc((void**)&h->w_noise, sizeof(float) * (size_t)h->cemb * h->cnoise))) return rc;
        if (c.label_dim && (rc = h->alloc((void**)&h->w_label, sizeof(float) * (size_t)h->cemb * c.label_dim))) return rc;
        if ((rc = h->alloc((void**)&h->w_mod, sizeof(float) * (size_t)h->total * h->cemb))) return rc;
        if ((rc = h->alloc((void**)&h->ones, sizeof(float2) * h->max_c))) return rc;
        std::vector<float2> one(h->max_c, make_float2(1.f, 0.f));
        HIP_TRY(hipMemcpy(h->ones, one.data(), sizeof(float2) * h->max_c, hipMemcpyHostToDevice));
        for (E2Block& b : h->dec)
            if (b.skip_c) {
                if ((rc = h->alloc((void**)&b.cat_ab, sizeof(float2) * b.cin))) return rc;
                std::vector<float2> v(b.cin);
                for (int i = 0; i < b.cin; ++i) v[i] = make_float2(i < b.cin - b.skip_c ? b.wa : b.wb, 0.f);
                HIP_TRY(hipMemcpy(b.cat_ab, v.data(), sizeof(float2) * b.cin, hipMemcpyHostToDevice));
            }
        h->device_ready = true;
    }
    const float k_silu = (float)(1.0 / 0.596);
    const double tr = c.res_balance, ta = c.attn_balance, tl = c.label_balance;
    const float res_main = (float)(tr / mp_sum_norm(tr)), attn_main = (float)(ta / mp_sum_norm(ta));
    // embedding: emb_noise (and emb_label with its sqrt(label_dim) input scale) with label_balance's mp_sum weights folded in
    const bool lab = c.label_dim != 0;
    HIP_TRY(edm2_launch_prep_weight(h->P(h->emb_noise), h->w_noise, h->cemb, h->cnoise, h->cnoise, 1, nullptr,
                                    lab ? (float)((1 - tl) / mp_sum_norm(tl)) : 1.f, 1.f, h->cnoise, s));
    if (lab)
        HIP_TRY(edm2_launch_prep_weight(h->P(h->emb_label), h->w_label, h->cemb, c.label_dim, c.label_dim, 1, nullptr,
                                        (float)(tl / mp_sum_norm(tl) * std::sqrt((double)c.label_dim)), 1.f, c.label_dim, s));
    if ((rc = e2_pack_conv(h, &h->p_stem, h->stem_w, h->stem_c, c.img_channels + 1, kE2StemPad, 3, nullptr, 1.f, 1.f, kE2StemPad, s))) return rc;
    for (auto* list : {&h->enc, &h->dec})
        for (E2Block& b : *list) {
            const int cin0 = b.enc ? b.cout : b.cin;
            if ((rc = e2_pack_conv(h, &b.p_res0, b.res0, b.cout, cin0, cin0, 3, nullptr, k_silu, k_silu, cin0, s))) return rc;
            if ((rc = e2_pack_conv(h, &b.p_res1, b.res1, b.cout, b.cout, b.cout, 3, nullptr, k_silu * res_main, 1.f, b.cout, s))) return rc;
            if (b.skip >= 0) {
                // decoder: mp_cat's weights fold into the skip conv's columns; encoder: a plain 1x1 conv
                const float e0 = b.skip_c ? b.wa : 1.f, e1 = b.skip_c ? b.wb : 1.f;
                if ((rc = e2_pack_conv(h, &b.p_skip, b.skip, b.cout, b.cin, b.cin, 1, nullptr, e0, e1, b.cin - b.skip_c, s))) return rc;
            }
            if (b.attn) {
                if ((rc = e2_pack_conv(h, &b.p_qkv, b.qkv, 3 * b.cout, b.cout, b.cout, 1, nullptr, 1.f, 1.f, b.cout, s))) return rc;
                if ((rc = e2_pack_conv(h, &b.p_proj, b.proj, b.cout, b.cout, b.cout, 1, nullptr, attn_main, 1.f, b.cout, s))) return rc;
            }
            HIP_TRY(edm2_launch_prep_weight(h->P(b.lin), h->w_mod + (size_t)b.off * h->cemb, b.cout, h->cemb, h->cemb, 1, h->P(b.gain), 1.f,
                                            1.f, h->cemb, s));
        }
    if ((rc = e2_pack_conv(h, &h->p_out, h->out_w, c.img_channels, h->out_cin, h->out_cin, 3, h->P(h->out_gain), 1.f, 1.f, h->out_cin, s)))
        return rc;
    return FG_OK;
}

// Block.forward (eval): resample; encoder: [conv_skip], pixel norm; y = conv_res1(mp_silu(conv_res0(mp_silu(x)) * c)); decoder:
// [conv_skip]; x = mp_sum(x, y, res_balance); [x = mp_sum(x, attn_proj(attention(attn_qkv(x))), attn_balance)]; clip.
int e2_block(fg_edm2* h, const E2Block& b, const float* x1, int c1, const float* x2, int c2, float* dst, int B, E2Ws& w, hipStream_t s) {
    const fg_edm2_config& c = h->cfg;
    const int Ho = b.res_out;
    const float clip = c.clip_act > 0 ? (float)c.clip_act : 0.f;
    const float res_skip = (float)((1 - c.res_balance) / mp_sum_norm(c.res_balance));
    const float attn_skip = (float)((1 - c.attn_balance) / mp_sum_norm(c.attn_balance));
    AdmConvArgs r0;
    r0.Hs = r0.H = Ho, r0.B = B, r0.silu = 1, r0.ab = h->ones, r0.ab_stride = 0;
    const float* resid = nullptr;
    int resid_mode = 0;
    if (b.enc) {
        if (b.skip >= 0) {
            AdmConvArgs k;
            k.src1 = x1, k.C1 = c1, k.Hs = k.H = Ho, k.B = B, k.w = b.p_skip, k.out = w.s, k.Cout = b.cout;
            HIP_TRY(adm_launch_conv(h->cmode, 1, k, s));
            HIP_TRY(edm2_launch_pixel_norm(w.s, w.s, B, Ho, b.cout, 0, s));
        } else {
            HIP_TRY(edm2_launch_pixel_norm(x1, w.s, B, Ho, b.cout, b.down ? 1 : 0, s));
        }
        r0.src1 = w.s, r0.C1 = b.cout;
        resid = w.s;
    } else if (b.up) {
        r0.src1 = x1, r0.C1 = c1, r0.Hs = b.res_in, r0.res_mode = 2;
        resid = x1, resid_mode = 2;
    } else if (c2) {
        r0.src1 = x1, r0.src2 = x2, r0.C1 = c1, r0.C2 = c2, r0.ab = b.cat_ab;
        AdmConvArgs k;
        k.src1 = x1, k.src2 = x2, k.C1 = c1, k.C2 = c2, k.Hs = k.H = Ho, k.B = B, k.w = b.p_skip, k.out = w.s, k.Cout = b.cout;
        HIP_TRY(adm_launch_conv(h->cmode, 1, k, s));
        resid = w.s;
    } else {
        r0.src1 = x1, r0.C1 = c1;
        resid = x1;
    }
    r0.w = b.p_res0, r0.out = w.h, r0.Cout = b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 3, r0, s));
    AdmConvArgs r1;
    r1.src1 = w.h, r1.C1 = b.cout, r1.Hs = r1.H = Ho, r1.B = B;
    r1.ab = w.ab_all + b.off, r1.ab_stride = h->total, r1.silu = 1, r1.w = b.p_res1;
    r1.resid = resid, r1.resid_mode = resid_mode, r1.resid_scale = res_skip;
    r1.clip = b.attn ? 0.f : clip, r1.out = b.attn ? w.t1 : dst, r1.Cout = b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 3, r1, s));
    if (!b.attn) return FG_OK;
    AdmConvArgs q;
    q.src1 = w.t1, q.C1 = b.cout, q.Hs = q.H = Ho, q.B = B, q.w = b.p_qkv, q.out = w.qkv, q.Cout = 3 * b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 1, q, s));
    HIP_TRY(adm_launch_attention_mp(w.qkv, w.a, B, Ho * Ho, b.cout / 64, s));
    AdmConvArgs p;
    p.src1 = w.a, p.C1 = b.cout, p.Hs = p.H = Ho, p.B = B, p.w = b.p_proj;
    p.resid = w.t1, p.resid_scale = attn_skip, p.clip = clip, p.out = dst, p.Cout = b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 1, p, s));
    return FG_OK;
}

// the conv_res1 prologue rows of every block from emb: c = emb_linear(emb, gain = emb_gain) + 1
int e2_modulation(fg_edm2* h, const float* emb, int B, E2Ws& w, hipStream_t s) {
    HIP_TRY(launch_linear(emb, h->w_mod, nullptr, w.cc, B, h->cemb, h->total, 0, s));
    HIP_TRY(edm2_launch_mod_rows(w.cc, w.ab_all, (int64_t)B * h->total, s));
    return FG_OK;
}

// EDM2Precond.forward (eval, x0) around EMD2UNet.forward
// taps (nullable): 2 + num_blocks nullable fp32 NHWC device buffers - the stem output, every block output in fg_edm2_block_info order,
// the raw U-Net output F - each copied on s behind the kernel that wrote it (fg_edm2_forward_taps).
int e2_forward(fg_edm2* h, const float* x_t, const double* t, int t_stride, const float* labels, float* out, int B, E2Ws& w, hipStream_t s,
               float* const* taps = nullptr) {
    const fg_edm2_config& c = h->cfg;
    int tap_i = 0;
    auto tap = [&](const float* src, int res, int ch) -> int {
        float* dst = taps ? taps[tap_i] : nullptr;
        ++tap_i;
        if (dst) HIP_TRY(hipMemcpyAsync(dst, src, sizeof(float) * (size_t)B * res * res * ch, hipMemcpyDeviceToDevice, s));
        return FG_OK;
    };
    HIP_TRY(launch_precond_coef(t, t_stride, nullptr, 0, c.sigma_data, h->shift(), 1e-6, c.drop_precond, w.coef, B, s));
    // embedding: mp_silu(mp_sum(emb_noise(fourier(c_noise)), emb_label(labels sqrt(L)), label_balance)), the balance folded in
    HIP_TRY(edm2_launch_fourier(w.coef + B, h->P(h->freqs), h->P(h->phases), w.four, B, h->cnoise, s));
    HIP_TRY(launch_linear(w.four, h->w_noise, nullptr, w.e, B, h->cnoise, h->cemb, 0, s));
    const bool lab = c.label_dim && labels;  // no labels: emb_label(zeros) = 0
    if (lab) HIP_TRY(launch_linear(labels, h->w_label, nullptr, w.lab, B, c.label_dim, h->cemb, 0, s));
    HIP_TRY(edm2_launch_emb_finish(w.e, lab ? w.lab : nullptr, w.emb, (int64_t)B * h->cemb, s));
    int rc;
    if ((rc = e2_modulation(h, w.emb, B, w, s))) return rc;
    // stem conv over [c_in x_t | ones]
    const int R = c.img_resolution;
    HIP_TRY(edm2_launch_stem_operand(x_t, w.coef, w.stem_in, B, c.img_channels, R, kE2StemPad, s));
    AdmConvArgs st;
    st.src1 = w.stem_in, st.C1 = kE2StemPad, st.Hs = st.H = R, st.B = B, st.w = h->p_stem, st.out = w.skip[0], st.Cout = h->stem_c;
    HIP_TRY(adm_launch_conv(h->cmode, 3, st, s));
    if ((rc = tap(w.skip[0], R, h->stem_c))) return rc;
    const float* x = w.skip[0];
    int xc = h->stem_c;
    for (size_t i = 0; i < h->enc.size(); ++i) {
        const E2Block& b = h->enc[i];
        if ((rc = e2_block(h, b, x, xc, nullptr, 0, w.skip[i + 1], B, w, s))) return rc;
        if ((rc = tap(w.skip[i + 1], b.res_out, b.cout))) return rc;
        x = w.skip[i + 1], xc = b.cout;
    }
    int sp = (int)w.skip.size();
    float* pong[2] = {w.xa, w.xb};
    int cur = 0;
    for (const E2Block& b : h->dec) {
        const float* x2 = b.skip_c ? w.skip[--sp] : nullptr;
        if ((rc = e2_block(h, b, x, xc, x2, b.skip_c, pong[cur], B, w, s))) return rc;
        if ((rc = tap(pong[cur], b.res_out, b.cout))) return rc;
        x = pong[cur], xc = b.cout;
        cur ^= 1;
    }
    AdmConvArgs o;
    o.src1 = x, o.C1 = h->out_cin, o.Hs = o.H = R, o.B = B, o.w = h->p_out, o.out = w.F, o.Cout = c.img_channels;
    HIP_TRY(adm_launch_conv(h->cmode, 3, o, s));
    if ((rc = tap(w.F, R, c.img_channels))) return rc;
    HIP_TRY(edm2_launch_precond_out(w.F, x_t, w.coef + 2 * (size_t)B, w.coef + 3 * (size_t)B, out, B, c.img_channels, R, s));
    return FG_OK;
}

const E2Block* e2_block_at(const fg_edm2* h, int index) {
    const int ne = (int)h->enc.size();
    if (index < 0 || index >= ne + (int)h->dec.size()) return nullptr;
    return index < ne ? &h->enc[index] : &h->dec[index - ne];
}

}  // namespace

extern "C" {

int fg_edm2_create(const fg_edm2_config* cfg, fg_edm2** out) {
    if (!cfg || !out) return fail(FG_EINVAL, "null argument");
    if (cfg->num_levels < 1 || cfg->num_levels > FG_MAX_LEVELS || cfg->num_attn_resolutions < 0 || cfg->num_attn_resolutions > FG_MAX_LEVELS)
        return fail(FG_EINVAL, "bad num_levels / num_attn_resolutions");
    if (cfg->compute_dtype != FG_DTYPE_BF16 && cfg->compute_dtype != FG_DTYPE_BF16X3)
        return fail(FG_EINVAL, "EDM2: compute_dtype must be FG_DTYPE_BF16X3 or FG_DTYPE_BF16 (the exact-fp32 mode is not implemented)");
    if (cfg->drop_precond & ~3) return fail(FG_EINVAL, "bad drop_precond");
    if (cfg->model_channels <= 0 || cfg->channel_mult_noise < 0 || cfg->channel_mult_emb < 0 || cfg->num_blocks < 0 || cfg->label_dim < 0)
        return fail(FG_EINVAL, "bad channel configuration");
    for (int i = 0; i < cfg->num_levels; ++i)
        if (cfg->channel_mult[i] <= 0) return fail(FG_EINVAL, "bad channel_mult");
    fg_edm2* h = new fg_edm2();
    h->cfg = *cfg;
    h->cmode = cfg->compute_dtype;
    e2_build_layout(h);
    const int rc = e2_check_supported(h);
    if (rc) {
        delete h;
        return rc;
    }
    *out = h;
    return FG_OK;
}

void fg_edm2_destroy(fg_edm2* h) {
    if (!h) return;
    h->sampler.release();
    delete h;
}

int fg_edm2_num_params(const fg_edm2* h) { return h ? (int)h->params.size() : 0; }

int fg_edm2_param_info(const fg_edm2* h, int index, const char** name, int* ndim, int64_t shape[4]) {
    return param_info(h, index, name, ndim, shape);
}

int fg_edm2_bind_param(fg_edm2* h, const char* name, const float* device_ptr, int64_t numel) {
    return bind_param(h, name, device_ptr, numel);
}

int fg_edm2_pack_weights(fg_edm2* h, void* stream) {
    if (!h) return fail(FG_EINVAL, "null handle");
    int rc = h->check_bound([](int) { return false; });
    if (rc || (rc = e2_pack(h, (hipStream_t)stream))) return rc;
    h->sampler.graph.drop();
    h->packed = true;
    return FG_OK;
}

size_t fg_edm2_workspace_bytes(const fg_edm2* h, int batch) {
    if (!h || batch <= 0) return 0;
    Arena A;
    A.dry = true;
    E2Ws w;
    return e2_plan(h, batch, A, w);
}

int fg_edm2_set_training(fg_edm2* h, int training) {
    if (!h) return fail(FG_EINVAL, "null handle");
    if ((training != 0) != h->training && h->cfg.sigma_shift != 0.0) h->sampler.graph.drop();  // a captured sampler baked the old shift in
    h->training = training != 0;
    return FG_OK;
}

int fg_edm2_num_taps(const fg_edm2* h) { return h ? 2 + (int)(h->enc.size() + h->dec.size()) : 0; }

int fg_edm2_forward_taps(fg_edm2* h, const float* x_t, const double* t, const float* class_labels, float* out, float* emb_out,
                         float* const* taps, int num_taps, int batch, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !x_t || !t || !out) return fail(FG_EINVAL, "null argument");
    if (taps && num_taps != fg_edm2_num_taps(h))
        return fail(FG_EINVAL, "fg_edm2_forward_taps: num_taps %d, the handle has %d (fg_edm2_num_taps)", num_taps, fg_edm2_num_taps(h));
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_edm2_pack_weights)");
    if (out == x_t) return fail(FG_EINVAL, "out must not alias x_t");
    for (int i = 0; taps && i < num_taps; ++i)
        if (taps[i] && (taps[i] == out || taps[i] == x_t || taps[i] == emb_out))
            return fail(FG_EINVAL, "fg_edm2_forward_taps: tap %d aliases x_t, out or emb_out", i);
    E2Ws w;
    int rc = setup_ws(e2_plan, h, batch, workspace, workspace_bytes, w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = e2_forward(h, x_t, t, 1, class_labels, out, batch, w, s, taps))) return rc;
    if (emb_out) HIP_TRY(hipMemcpyAsync(emb_out, w.emb, sizeof(float) * (size_t)batch * h->cemb, hipMemcpyDeviceToDevice, s));
    return FG_OK;
}

int fg_edm2_forward(fg_edm2* h, const float* x_t, const double* t, const float* class_labels, float* out, float* emb_out, int batch,
                    void* workspace, size_t workspace_bytes, void* stream) {
    return fg_edm2_forward_taps(h, x_t, t, class_labels, out, emb_out, nullptr, 0, batch, workspace, workspace_bytes, stream);
}

int fg_edm2_sampler_run(fg_edm2* h, const float* noise, const float* class_labels, const double* t_list, int steps, int sample_type,
                        int loop_kind, const float* eps, uint64_t seed, float* out, int batch, void* workspace, size_t workspace_bytes,
                        int use_graph, void* stream) {
    if (!h || !noise || !t_list || !out) return fail(FG_EINVAL, "null argument");
    int rc = check_sampler_args(t_list, steps, sample_type, loop_kind, FG_SCHEDULE_EDM);
    if (rc) return rc;
    if (loop_kind != FG_LOOP_X0) return fail(FG_EINVAL, "EDM2 runs the FG_LOOP_X0 loop only");
    E2Ws w;
    if ((rc = setup_ws(e2_plan, h, batch, workspace, workspace_bytes, w))) return rc;
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_edm2_pack_weights)");
    const int64_t total = (int64_t)batch * h->cfg.img_channels * h->cfg.img_resolution * h->cfg.img_resolution;
    return sampler_launch(h->sampler, batch, t_list, steps, sample_type, loop_kind, seed, w.tl, w.seed, use_graph,
                          {(int64_t)(uintptr_t)noise, (int64_t)(uintptr_t)class_labels, (int64_t)(uintptr_t)eps, (int64_t)(uintptr_t)out,
                           (int64_t)(uintptr_t)workspace},
                          (hipStream_t)stream, [&](hipStream_t q) {
                              const StudentLoop L{noise, t_list, steps, sample_type, FG_SCHEDULE_EDM, total, w.x, w.eps, eps, w.tl, w.seed, out, q};
                              return x0_loop(L, w.x_pred, [&](int i, float* pred) { return e2_forward(h, w.x, w.tl + i, 0, class_labels, pred, batch, w, q); });
                          });
}

int fg_edm2_num_blocks(const fg_edm2* h) { return h ? (int)(h->enc.size() + h->dec.size()) : 0; }

int fg_edm2_block_info(const fg_edm2* h, int index, const char** key, int* cin, int* cout, int* res_in, int* res_out, int* has_attention) {
    if (!h) return fail(FG_EINVAL, "null handle");
    const E2Block* b = e2_block_at(h, index);
    if (!b) return fail(FG_EINVAL, "block index out of range");
    if (key) *key = b->key.c_str();
    if (cin) *cin = b->cin;
    if (cout) *cout = b->cout;
    if (res_in) *res_in = b->res_in;
    if (res_out) *res_out = b->res_out;
    if (has_attention) *has_attention = b->attn ? 1 : 0;
    return FG_OK;
}

int fg_edm2_run_block(fg_edm2* h, int index, const float* x1, int c1, const float* x2, int c2, const float* emb, float* out, int batch,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !x1 || !emb || !out) return fail(FG_EINVAL, "null argument");
    const E2Block* b = e2_block_at(h, index);
    if (!b) return fail(FG_EINVAL, "block index out of range");
    if (c1 <= 0 || c2 != b->skip_c || c1 + c2 != b->cin)
        return fail(FG_EINVAL, "%s: channel split c1 = %d, c2 = %d; the block takes %d + %d (its skip)", b->key.c_str(), c1, c2,
                    b->cin - b->skip_c, b->skip_c);
    if (c2 && !x2) return fail(FG_EINVAL, "%s: x2 is null", b->key.c_str());
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_edm2_pack_weights)");
    E2Ws w;
    int rc = setup_ws(e2_plan, h, batch, workspace, workspace_bytes, w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = e2_modulation(h, emb, batch, w, s))) return rc;
    return e2_block(h, *b, x1, c1, c2 ? x2 : nullptr, c2, out, batch, w, s);
}
