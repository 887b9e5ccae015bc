// DhariwalUNet (ADM) engine: module layout and state-dict order, weight packing, workspace plan and the forward schedule of
// EDMPrecond(model_type="DhariwalUNet") (reference fastgen/networks/EDM/network.py:584-740 with UNetBlock :205-303).  Included by
// engine.hip inside its anonymous namespace; kernels in adm.hip.  Forward only, split-bf16 and bf16 convolutions.

struct AdmBlock {
    std::string key;
    int cin = 0, cout = 0, res_in = 0, res_out = 0;
    bool up = false, down = false, attn = false;
    int skip_c = 0;    // decoder: channels taken from the skip stack (concat), else 0
    int temb_off = 0;  // column of this block's affine() (2 cout: scale, shift) in the stacked embedding projection
    int norm0_w = -1, norm0_b = -1, conv0_w = -1, conv0_b = -1, aff_w = -1, aff_b = -1, norm1_w = -1, norm1_b = -1, conv1_w = -1,
        conv1_b = -1, skip_w = -1, skip_b = -1, norm2_w = -1, norm2_b = -1, qkv_w = -1, qkv_b = -1, proj_w = -1, proj_b = -1;
    void *p_conv0 = nullptr, *p_conv1 = nullptr, *p_skip = nullptr, *p_qkv = nullptr, *p_proj = nullptr;
};

struct AdmNet {
    int map_aug = -1, map0_w = -1, map0_b = -1, map1_w = -1, map1_b = -1, map_label = -1;
    int stem_w = -1, stem_b = -1, stem_c = 0;
    int out_norm_w = -1, out_norm_b = -1, out_conv_w = -1, out_conv_b = -1, out_cin = 0;
    std::vector<AdmBlock> enc, dec;
    std::vector<int> skip_c, skip_res;  // channels / resolution of every encoder output (stem first): the skip stack
    float* freqs = nullptr;             // [model_channels / 2] PositionalEmbedding(endpoint=False) frequencies
};

constexpr float kAdmEps = 1e-5f;  // UNetBlock / GroupNorm default eps (EDM/network.py:134, 218)

void adm_build_layout(fg_edm* h) {
    const fg_edm_config& c = h->cfg;
    AdmNet* n = h->adm;
    const int E = h->emb_ch, N = h->cond_ch, mc = c.model_channels;
    if (c.augment_dim) n->map_aug = h->add("model.map_augment.weight", {N, c.augment_dim});
    n->map0_w = h->add("model.map_layer0.weight", {E, N});
    n->map0_b = h->add("model.map_layer0.bias", {E});
    n->map1_w = h->add("model.map_layer1.weight", {E, E});
    n->map1_b = h->add("model.map_layer1.bias", {E});
    if (c.label_dim) n->map_label = h->add("model.map_label.weight", {E, c.label_dim});
    auto attn_at = [&](int res) {
        for (int i = 0; i < c.num_attn_resolutions; ++i)
            if (c.attn_resolutions[i] == res) return true;
        return false;
    };
    auto add_block = [&](const std::string& key, int cin, int cout, int res_in, int res_out, bool up, bool down, bool attn) {
        AdmBlock b;
        b.key = key;
        b.cin = cin, b.cout = cout, b.res_in = res_in, b.res_out = res_out, b.up = up, b.down = down, b.attn = attn;
        const std::string p = key + ".";
        b.norm0_w = h->add(p + "norm0.weight", {cin});
        b.norm0_b = h->add(p + "norm0.bias", {cin});
        b.conv0_w = h->add(p + "conv0.weight", {cout, cin, 3, 3});
        b.conv0_b = h->add(p + "conv0.bias", {cout});
        b.aff_w = h->add(p + "affine.weight", {2 * cout, E});
        b.aff_b = h->add(p + "affine.bias", {2 * cout});
        b.norm1_w = h->add(p + "norm1.weight", {cout});
        b.norm1_b = h->add(p + "norm1.bias", {cout});
        b.conv1_w = h->add(p + "conv1.weight", {cout, cout, 3, 3});
        b.conv1_b = h->add(p + "conv1.bias", {cout});
        if (cin != cout) {  // up / down blocks keep the width: their skip is the weightless resample (kernel 0)
            b.skip_w = h->add(p + "skip.weight", {cout, cin, 1, 1});
            b.skip_b = h->add(p + "skip.bias", {cout});
        }
        if (attn) {
            b.norm2_w = h->add(p + "norm2.weight", {cout});
            b.norm2_b = h->add(p + "norm2.bias", {cout});
            b.qkv_w = h->add(p + "qkv.weight", {3 * cout, cout, 1, 1});
            b.qkv_b = h->add(p + "qkv.bias", {3 * cout});
            b.proj_w = h->add(p + "proj.weight", {cout, cout, 1, 1});
            b.proj_b = h->add(p + "proj.bias", {cout});
        }
        b.temb_off = h->temb_total;
        h->temb_total += 2 * cout;
        return b;
    };
    // encoder (:656-673)
    int cout = c.img_channels;
    for (int level = 0; level < c.num_levels; ++level) {
        const int res = c.img_resolution >> level;
        const std::string r = "model.enc." + std::to_string(res) + "x" + std::to_string(res);
        if (level == 0) {
            n->stem_c = mc * c.channel_mult[level];
            n->stem_w = h->add(r + "_conv.weight", {n->stem_c, cout, 3, 3});
            n->stem_b = h->add(r + "_conv.bias", {n->stem_c});
            cout = n->stem_c;
            n->skip_c.push_back(cout), n->skip_res.push_back(res);
        } else {
            n->enc.push_back(add_block(r + "_down", cout, cout, 2 * res, res, false, true, false));
            n->skip_c.push_back(cout), n->skip_res.push_back(res);
        }
        for (int i = 0; i < c.num_blocks; ++i) {
            const int cin = cout;
            cout = mc * c.channel_mult[level];
            n->enc.push_back(add_block(r + "_block" + std::to_string(i), cin, cout, res, res, false, false, attn_at(res)));
            n->skip_c.push_back(cout), n->skip_res.push_back(res);
        }
    }
    // decoder (:676-691)
    std::vector<int> skips = n->skip_c;
    for (int level = c.num_levels - 1; level >= 0; --level) {
        const int res = c.img_resolution >> level;
        const std::string r = "model.dec." + std::to_string(res) + "x" + std::to_string(res);
        if (level == c.num_levels - 1) {
            n->dec.push_back(add_block(r + "_in0", cout, cout, res, res, false, false, true));
            n->dec.push_back(add_block(r + "_in1", cout, cout, res, res, false, false, false));
        } else {
            n->dec.push_back(add_block(r + "_up", cout, cout, res / 2, res, true, false, false));
        }
        for (int i = 0; i <= c.num_blocks; ++i) {
            const int sc = skips.back();
            skips.pop_back();
            const int cin = cout + sc;
            cout = mc * c.channel_mult[level];
            n->dec.push_back(add_block(r + "_block" + std::to_string(i), cin, cout, res, res, false, false, attn_at(res)));
            n->dec.back().skip_c = sc;
        }
    }
    n->out_cin = cout;
    n->out_norm_w = h->add("model.out_norm.weight", {cout});
    n->out_norm_b = h->add("model.out_norm.bias", {cout});
    n->out_conv_w = h->add("model.out_conv.weight", {c.img_channels, cout, 3, 3});
    n->out_conv_b = h->add("model.out_conv.bias", {c.img_channels});
    h->add("model.logvar_linear.weight", {1, mc});
    h->add("model.logvar_linear.bias", {1});
}

int adm_check_supported(const fg_edm* h) {
    const fg_edm_config& c = h->cfg;
    const AdmNet* n = h->adm;
    if (h->cmode == FG_DTYPE_F32) return fail(FG_EINVAL, "DhariwalUNet: the exact-fp32 mode is not implemented (bf16x3 or bf16)");
    if (c.r_timestep) return fail(FG_EINVAL, "DhariwalUNet: r_timestep is not implemented");
    const int R = c.img_resolution;
    if (R > 64 || R < 8 || (R & (R - 1))) return fail(FG_EINVAL, "DhariwalUNet: img_resolution %d unsupported (8 .. 64, power of two)", R);
    if ((R >> (c.num_levels - 1)) < 8) return fail(FG_EINVAL, "DhariwalUNet: lowest resolution %d < 8 unsupported", R >> (c.num_levels - 1));
    if (c.img_channels < 1 || c.img_channels > 4) return fail(FG_EINVAL, "DhariwalUNet: img_channels %d unsupported (1 .. 4)", c.img_channels);
    if (c.model_channels % 4) return fail(FG_EINVAL, "DhariwalUNet: model_channels must be a multiple of 4");
    for (int i = 0; i < c.num_levels; ++i)
        if ((c.model_channels * c.channel_mult[i]) % 64)
            return fail(FG_EINVAL, "DhariwalUNet: level %d has %d channels, not a multiple of 64", i, c.model_channels * c.channel_mult[i]);
    if ((size_t)c.img_channels * 9 * n->stem_c * 4 > 64 * 1024) return fail(FG_EINVAL, "DhariwalUNet: stem too wide");
    if ((size_t)9 * c.img_channels * n->out_cin * 4 + (size_t)n->out_cin * 8 > 64 * 1024) return fail(FG_EINVAL, "DhariwalUNet: output head too wide");
    for (const auto* list : {&n->enc, &n->dec})
        for (const AdmBlock& b : *list)
            if (b.attn && (b.res_out > 32 || (b.res_out * b.res_out) % 64))
                return fail(FG_EINVAL, "%s: attention at %dx%d unsupported (8x8 .. 32x32)", b.key.c_str(), b.res_out, b.res_out);
    return FG_OK;
}

struct AdmPlanSizes {
    size_t max_act = 0, max_attn = 0, max_part = 0;
    int max_c = 0;
};

AdmPlanSizes adm_sizes(const fg_edm* h, int B) {
    const AdmNet* n = h->adm;
    AdmPlanSizes z;
    for (const auto* list : {&n->enc, &n->dec})
        for (const AdmBlock& b : *list) {
            const size_t hw = (size_t)b.res_out * b.res_out;
            z.max_act = std::max(z.max_act, hw * b.cout);
            z.max_c = std::max(z.max_c, std::max(b.cin, b.cout));
            if (b.attn) z.max_attn = std::max(z.max_attn, hw * b.cout);
            z.max_part = std::max(z.max_part, adm_gn_part_elems(B, b.res_in * b.res_in, b.cin));
            z.max_part = std::max(z.max_part, adm_gn_part_elems(B, b.res_out * b.res_out, b.cout));
        }
    const int R = h->cfg.img_resolution;
    z.max_part = std::max(z.max_part, adm_gn_part_elems(B, R * R, n->out_cin));
    return z;
}

size_t adm_plan_workspace(const fg_edm* h, int B, Arena& A, Workspace& w) {
    const fg_edm_config& c = h->cfg;
    const AdmNet* n = h->adm;
    const AdmPlanSizes z = adm_sizes(h, B);
    AdmWs& q = w.adm;
    w.coef = A.get<float>(5 * (size_t)B);
    w.emb0 = A.get<float>((size_t)B * h->cond_ch);
    w.emb1 = A.get<float>((size_t)B * h->emb_ch);
    q.e2 = A.get<float>((size_t)B * h->emb_ch);
    q.lab = A.get<float>((size_t)B * h->emb_ch);
    w.emb = A.get<float>((size_t)B * h->emb_ch);
    w.temb = A.get<float>((size_t)B * h->temb_total);
    w.ab0 = A.get<float2>((size_t)B * z.max_c);
    q.part = A.get<float2>(z.max_part);
    q.skip.clear();
    for (size_t i = 0; i < n->skip_c.size(); ++i) q.skip.push_back(A.get<float>((size_t)B * n->skip_res[i] * n->skip_res[i] * n->skip_c[i]));
    q.xa = A.get<float>((size_t)B * z.max_act);
    q.xb = A.get<float>((size_t)B * z.max_act);
    q.h = A.get<float>((size_t)B * z.max_act);
    q.s = A.get<float>((size_t)B * z.max_act);
    q.t1 = A.get<float>((size_t)B * std::max(z.max_attn, (size_t)1));
    q.qkv = A.get<float>((size_t)B * 3 * std::max(z.max_attn, (size_t)1));
    q.a = A.get<float>((size_t)B * std::max(z.max_attn, (size_t)1));
    const size_t img = (size_t)B * c.img_channels * c.img_resolution * c.img_resolution;
    w.x = A.get<float>(img);
    w.x_pred = A.get<float>(img);
    w.eps = A.get<float>(img);
    w.tl = A.get<double>(ScalarRing::kDoubles);
    w.seed = A.get<uint64_t>(8);
    return (A.off + 255) & ~(size_t)255;
}

int adm_pack_weights(fg_edm* h, hipStream_t s) {
    AdmNet* n = h->adm;
    int rc;
    const int mode = h->cmode;
    auto pack = [&](void** dst, int widx, int cout, int cin, int ks) -> int {
        if (!*dst && (rc = h->alloc(dst, adm_conv_pack_elems(mode, cout, cin, ks) * sizeof(__bf16)))) return rc;
        HIP_TRY(adm_pack_conv_weights(mode, h->P(widx), *dst, cout, cin, ks, s));
        return FG_OK;
    };
    if (!h->device_ready) {
        if ((rc = h->alloc((void**)&h->aff_w, sizeof(float) * (size_t)h->temb_total * h->emb_ch))) return rc;
        if ((rc = h->alloc((void**)&h->aff_b, sizeof(float) * (size_t)h->temb_total))) return rc;
        // PositionalEmbedding(num_channels=model_channels), endpoint=False (EDM/network.py:306-319): (1/10000)^(j / half)
        const int half = h->cond_ch / 2;
        std::vector<float> fr(half);
        for (int j = 0; j < half; ++j) fr[j] = powf(1.0f / 10000.0f, (float)j / (float)half);
        if ((rc = h->alloc((void**)&n->freqs, sizeof(float) * half))) return rc;
        HIP_TRY(hipMemcpy(n->freqs, fr.data(), sizeof(float) * half, hipMemcpyHostToDevice));
        h->device_ready = true;
    }
    for (auto* list : {&n->enc, &n->dec})
        for (AdmBlock& b : *list) {
            if ((rc = pack(&b.p_conv0, b.conv0_w, b.cout, b.cin, 3))) return rc;
            if ((rc = pack(&b.p_conv1, b.conv1_w, b.cout, b.cout, 3))) return rc;
            if (b.skip_w >= 0 && (rc = pack(&b.p_skip, b.skip_w, b.cout, b.cin, 1))) return rc;
            if (b.attn) {
                if ((rc = pack(&b.p_qkv, b.qkv_w, 3 * b.cout, b.cout, 1))) return rc;
                if ((rc = pack(&b.p_proj, b.proj_w, b.cout, b.cout, 1))) return rc;
            }
            HIP_TRY(hipMemcpyAsync(h->aff_w + (size_t)b.temb_off * h->emb_ch, h->P(b.aff_w), sizeof(float) * (size_t)2 * b.cout * h->emb_ch,
                                   hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(h->aff_b + b.temb_off, h->P(b.aff_b), sizeof(float) * 2 * b.cout, hipMemcpyDeviceToDevice, s));
        }
    return FG_OK;
}

// UNetBlock.forward with adaptive_scale=True, skip_scale=1 (EDM/network.py:274-299):
//   h = conv0(silu(norm0(x)));  h = conv1(silu(shift + norm1(h) (scale + 1))) + skip(x);  [attention: h = proj(attn(qkv(norm2(h)))) + h]
int adm_block(fg_edm* h, const AdmBlock& b, const float* x1, int c1, const float* x2, int c2, float* dst, int B, Workspace& w,
              hipStream_t s) {
    AdmWs& q = w.adm;
    const int hw_in = b.res_in * b.res_in, hw = b.res_out * b.res_out;
    HIP_TRY(adm_launch_gn(x1, c1, x2, c2, h->P(b.norm0_w), h->P(b.norm0_b), kAdmEps, nullptr, 0, q.part, w.ab0, B, hw_in, s));
    AdmConvArgs a;
    a.src1 = x1, a.src2 = x2, a.C1 = c1, a.C2 = c2, a.Hs = b.res_in, a.H = b.res_out, a.B = B;
    a.res_mode = b.down ? 1 : b.up ? 2 : 0;
    a.ab = w.ab0, a.silu = 1, a.w = b.p_conv0, a.bias = h->P(b.conv0_b), a.out = q.h, a.Cout = b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 3, a, s));
    // norm1 with the block's affine(emb) = [scale | shift] folded into the coefficients
    HIP_TRY(adm_launch_gn(q.h, b.cout, nullptr, 0, h->P(b.norm1_w), h->P(b.norm1_b), kAdmEps, w.temb + b.temb_off, h->temb_total, q.part,
                          w.ab0, B, hw, s));
    const float* resid = x1;
    int resid_mode = b.down ? 1 : b.up ? 2 : 0;
    if (b.skip_w >= 0) {
        AdmConvArgs k;
        k.src1 = x1, k.src2 = x2, k.C1 = c1, k.C2 = c2, k.Hs = k.H = b.res_out, k.B = B;
        k.w = b.p_skip, k.bias = h->P(b.skip_b), k.out = q.s, k.Cout = b.cout;
        HIP_TRY(adm_launch_conv(h->cmode, 1, k, s));
        resid = q.s, resid_mode = 0;
    }
    AdmConvArgs d;
    d.src1 = q.h, d.C1 = b.cout, d.Hs = d.H = b.res_out, d.B = B;
    d.ab = w.ab0, d.silu = 1, d.w = b.p_conv1, d.bias = h->P(b.conv1_b), d.resid = resid, d.resid_mode = resid_mode;
    d.out = b.attn ? q.t1 : dst, d.Cout = b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 3, d, s));
    if (!b.attn) return FG_OK;
    HIP_TRY(adm_launch_gn(q.t1, b.cout, nullptr, 0, h->P(b.norm2_w), h->P(b.norm2_b), kAdmEps, nullptr, 0, q.part, w.ab0, B, hw, s));
    AdmConvArgs e;
    e.src1 = q.t1, e.C1 = b.cout, e.Hs = e.H = b.res_out, e.B = B;
    e.ab = w.ab0, e.silu = 0, e.w = b.p_qkv, e.bias = h->P(b.qkv_b), e.out = q.qkv, e.Cout = 3 * b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 1, e, s));
    HIP_TRY(adm_launch_attention(q.qkv, q.a, B, hw, b.cout / 64, s));
    AdmConvArgs f;
    f.src1 = q.a, f.C1 = b.cout, f.Hs = f.H = b.res_out, f.B = B;
    f.w = b.p_proj, f.bias = h->P(b.proj_b), f.resid = q.t1, f.resid_mode = 0, f.out = dst, f.Cout = b.cout;
    HIP_TRY(adm_launch_conv(h->cmode, 1, f, s));
    return FG_OK;
}

// EDMPrecond.forward (eval, fwd_pred_type = net_pred_type) around DhariwalUNet.forward (EDM/network.py:693-740, 881-974)
int adm_forward(fg_edm* h, const float* x_t, const double* t, int t_stride, const float* labels, float* out, int B, Workspace& w,
                hipStream_t s) {
    const fg_edm_config& c = h->cfg;
    const AdmNet* n = h->adm;
    AdmWs& q = w.adm;
    HIP_TRY(launch_precond_coef(t, t_stride, nullptr, 0, c.sigma_data, h->shift(), 1e-6, c.drop_precond, w.coef, B, s));
    // mapping: silu(map_layer1(silu(map_layer0(posemb(c_noise) [+ map_augment(aug)]))) + map_label(labels))
    HIP_TRY(adm_launch_map_in(w.coef + B, n->freqs, h->augment, h->augment ? h->P(n->map_aug) : nullptr, c.augment_dim, w.emb0, B,
                              h->cond_ch, s));
    HIP_TRY(launch_linear(w.emb0, h->P(n->map0_w), h->P(n->map0_b), w.emb1, B, h->cond_ch, h->emb_ch, 1, s));
    HIP_TRY(launch_linear(w.emb1, h->P(n->map1_w), h->P(n->map1_b), q.e2, B, h->emb_ch, h->emb_ch, 0, s));
    const bool lab = c.label_dim && labels;  // no labels: map_label(zeros) = 0 (no bias)
    if (lab) HIP_TRY(launch_linear(labels, h->P(n->map_label), nullptr, q.lab, B, c.label_dim, h->emb_ch, 0, s));
    HIP_TRY(adm_launch_add_silu(q.e2, lab ? q.lab : nullptr, w.emb, (int64_t)B * h->emb_ch, s));
    HIP_TRY(launch_linear(w.emb, h->aff_w, h->aff_b, w.temb, B, h->emb_ch, h->temb_total, 0, s));
    // encoder: stem conv3x3(c_in x_t) + bias, then the blocks; every output stays on the skip stack
    const int R = c.img_resolution;
    HIP_TRY(launch_conv_in(0, x_t, w.coef, h->P(n->stem_w), h->P(n->stem_b), q.skip[0], B, R, c.img_channels, n->stem_c, s));
    const float* x = q.skip[0];
    int rc;
    for (size_t i = 0; i < n->enc.size(); ++i) {
        const AdmBlock& b = n->enc[i];
        if ((rc = adm_block(h, b, x, b.cin, nullptr, 0, q.skip[i + 1], B, w, s))) return rc;
        x = q.skip[i + 1];
    }
    // decoder: the concat with the popped skip is virtual (two source pointers)
    int sp = (int)q.skip.size();
    float* pong[2] = {q.xa, q.xb};
    int cur = 0;
    for (const AdmBlock& b : n->dec) {
        const float* x2 = b.skip_c ? q.skip[--sp] : nullptr;
        if ((rc = adm_block(h, b, x, b.cin - b.skip_c, x2, b.skip_c, pong[cur], B, w, s))) return rc;
        x = pong[cur];
        cur ^= 1;
    }
    // out_conv(silu(out_norm(x))) and precond_output
    HIP_TRY(adm_launch_gn(x, n->out_cin, nullptr, 0, h->P(n->out_norm_w), h->P(n->out_norm_b), kAdmEps, nullptr, 0, q.part, w.ab0, B,
                          R * R, s));
    HIP_TRY(launch_aux_out(0, x, w.ab0, h->P(n->out_conv_w), h->P(n->out_conv_b), x_t, w.coef, out, B, R, n->out_cin, c.img_channels, s));
    return FG_OK;
}

// fg_edm_num_blocks / fg_edm_block_info / fg_edm_run_block on an ADM handle: the encoder blocks, then the decoder blocks.
int adm_num_blocks(const fg_edm* h) { return (int)(h->adm->enc.size() + h->adm->dec.size()); }

const AdmBlock* adm_block_at(const fg_edm* h, int index) {
    const AdmNet* n = h->adm;
    const int ne = (int)n->enc.size();
    if (index < 0 || index >= adm_num_blocks(h)) return nullptr;
    return index < ne ? &n->enc[index] : &n->dec[index - ne];
}

int adm_block_info(const fg_edm* h, int index, const char** key, int* cin, int* cout, int* res_in, int* res_out, int* has_attention) {
    const AdmBlock* b = adm_block_at(h, index);
    if (!b) return fail(FG_EINVAL, "block index out of range");
    if (key) *key = b->key.c_str();
    if (cin) *cin = b->cin;
    if (cout) *cout = b->cout;
    if (res_in) *res_in = b->res_in;
    if (res_out) *res_out = b->res_out;
    if (has_attention) *has_attention = b->attn ? 1 : 0;
    return FG_OK;
}

// One block on caller tensors (fp32 NHWC, as the network keeps them): temb = affine(emb) as adm_forward computes it, then adm_block.
int adm_run_block(fg_edm* h, int index, const float* x1, int c1, const float* x2, int c2, const float* emb, float* out, int B,
                  void* workspace, size_t workspace_bytes, hipStream_t s) {
    const AdmBlock* b = adm_block_at(h, index);
    if (!b) return fail(FG_EINVAL, "block index out of range");
    if (c1 <= 0 || c2 != b->skip_c || c1 + c2 != b->cin)
        return fail(FG_EINVAL, "%s: channel split c1 = %d, c2 = %d; the block takes %d + %d (its skip)", b->key.c_str(), c1, c2,
                    b->cin - b->skip_c, b->skip_c);
    if (c2 && !x2) return fail(FG_EINVAL, "%s: x2 is null", b->key.c_str());
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_edm_pack_weights)");
    Workspace w;
    int rc = setup_ws(plan_workspace, h, B, workspace, workspace_bytes, w);
    if (rc) return rc;
    HIP_TRY(launch_linear(emb, h->aff_w, h->aff_b, w.temb, B, h->emb_ch, h->temb_total, 0, s));
    return adm_block(h, *b, x1, c1, c2 ? x2 : nullptr, c2, out, B, w, s);
}
