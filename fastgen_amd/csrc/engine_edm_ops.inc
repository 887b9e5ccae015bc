// fg_op_edm_* entry points over the launchers of the SongUNet (EDMPrecond) INFERENCE kernels - conv.hip, conv_ws.hip, conv_ws3.hip, the
// GroupNorm finalize / pool / stem / head kernels of misc.hip and aux.hip, attn.hip: no engine handle, device pointers.  Each checks
// every argument first - a shape, alignment, null pointer or combination the launcher cannot serve is FG_EINVAL with its reason in
// fg_last_error(), before anything is launched - and then calls the launcher run_block / run_forward (engine.hip) call, so a per-op
// test runs the production kernels through the production dispatch.  Included by engine.hip.

namespace {

bool al16(const void* p) { return !(((uintptr_t)p) & 15); }
bool al8(const void* p) { return !(((uintptr_t)p) & 7); }
int edm_storage(int dtype) { return dtype == FG_DTYPE_BF16 ? 1 : 0; }  // the bf16x3 mode keeps fp32 tensors

// the (ks, pro, res, outmode) instantiations of launch_t (conv.hip): what conv_fused_kernel is built for
bool edm_conv_generic_form(int dtype, int ks, int pro, int res, int outmode, int W) {
    if (outmode == OUT_QKV) return ks == 1 && pro == PRO_GN && res == RES_NONE;
    if (outmode == OUT_QV) return dtype == FG_DTYPE_BF16X3 && ks == 1 && pro == PRO_GN && res == RES_NONE && W == 16;
    if (ks == 3 && pro == PRO_GN_SILU) return res == RES_NONE || res == RES_UP;
    if (ks == 3 && pro == PRO_NONE) return res == RES_NONE;
    if (ks == 1 && pro == PRO_NONE) return res == RES_NONE || res == RES_DOWN || res == RES_UP;
    return false;
}

// Shape part of a conv call: fills the ConvArgs fields the dispatch predicates read and names what is wrong (nullptr: nothing).
const char* edm_conv_shape(int dtype, int ks, int pro, int res, int outmode, int c1, int c2, int batch, int hs, int h, int cout, int rshift,
                           ConvArgs& a) {
    if (dtype != FG_DTYPE_F32 && dtype != FG_DTYPE_BF16 && dtype != FG_DTYPE_BF16X3) return "dtype must be 0 (fp32), 1 (bf16) or 2 (bf16x3)";
    if (ks != 1 && ks != 3) return "ks must be 1 or 3";
    if (pro != PRO_NONE && pro != PRO_GN && pro != PRO_GN_SILU) return "pro must be 0 (none), 1 (a x + b) or 2 (silu(a x + b))";
    if (res != RES_NONE && res != RES_DOWN && res != RES_UP && res != RES_SUBPIX) return "res must be 0 (none), 1 (down), 2 (up) or 3 (sub-pixel up)";
    if (outmode != OUT_NHWC && outmode != OUT_QKV && outmode != OUT_QV) return "outmode must be 0 (NHWC), 1 (q | k | v^T planes) or 4 (q' | v'^T planes)";
    if (h != 8 && h != 16 && h != 32) return "the output resolution must be 8, 16 or 32";
    if ((res == RES_NONE && hs != h) || (res == RES_DOWN && hs != 2 * h) || ((res == RES_UP || res == RES_SUBPIX) && 2 * hs != h))
        return "the source resolution must be h (res 0), 2 h (res 1) or h / 2 (res 2, 3)";
    const int kc = dtype == FG_DTYPE_BF16 ? 64 : 32;
    if (c1 <= 0 || c2 < 0 || (c1 % kc) || (c2 % kc)) return "c1 > 0 and c2 >= 0 must be multiples of the K step (64 in bf16, else 32)";
    if (batch <= 0 || batch > 65535) return "batch must be 1 .. 65535";
    if (outmode == OUT_NHWC && (cout <= 0 || (cout % 256))) return "cout must be a positive multiple of 256";
    if (outmode == OUT_QKV && (cout != 768 || h > 16)) return "the q | k | v^T form needs cout 768 at 8x8 or 16x16";
    if (outmode == OUT_QV && (cout != 512 || h != 16 || dtype != FG_DTYPE_BF16X3)) return "the q' | v'^T form needs cout 512 at 16x16 in bf16x3";
    if (rshift != 0 && rshift != 1) return "rshift must be 0 or 1";
    a.C1 = c1, a.C2 = c2, a.Hs = a.Ws = hs, a.H = a.W = h, a.B = batch, a.Cout = cout, a.rshift = rshift;
    return nullptr;
}

// Which kernel launch_conv_fused takes for `a` (its own two tests, in its order) and how many statistics slots per image it writes;
// 0: no kernel serves the call.
int edm_conv_kernel(int dtype, int ks, int pro, int res, int outmode, const ConvArgs& a, int* slots) {
    int kernel = 0;
    // the shifted residual is conv3_x3ws_kernel's alone: conv_ws_supported does not look at rshift (the engine sets it in bf16x3 only)
    if (a.rshift && !(dtype == FG_DTYPE_BF16X3 && conv_ws_enabled() && conv_x3ws_supported(ks, pro, res, outmode, a)))
        kernel = 0;
    else if (conv_ws_enabled() && conv_ws_supported(dtype, ks, pro, res, outmode, a)) {
        // launch_conv_ws builds the four-step form (128 input channels) for 32x32 without resampling only and returns an error
        // for the others, which conv_ws_supported lets through: no kernel, refused here before the launch
        const bool four_steps = pro != PRO_NONE && (a.C1 + a.C2) / 32 == 4;
        kernel = (four_steps && (res != RES_NONE || a.W != 32)) ? 0 : FG_EDM_CONV_WS;
    }
    else if (dtype == FG_DTYPE_BF16X3 && conv_ws_enabled() && conv_x3ws_supported(ks, pro, res, outmode, a))
        kernel = FG_EDM_CONV_X3WS;
    else if (res != RES_SUBPIX && !a.rshift && edm_conv_generic_form(dtype, ks, pro, res, outmode, a.W))
        kernel = FG_EDM_CONV_GENERIC;
    if (slots) *slots = kernel ? conv_launch_stat_slots(dtype, ks, pro, res, outmode, a) : 0;
    return kernel;
}

bool edm_gn_ok(int c1, int c2) {
    const int C = c1 + c2;
    if (c1 <= 0 || c2 < 0 || (c1 % 4) || (c2 % 4) || C < 16 || C > 512) return false;
    const int groups = C / 4 < 32 ? C / 4 : 32;
    return !(C % groups) && !((C / groups) % 4);
}

}  // namespace

size_t fg_op_edm_conv_pack_bytes(int dtype, int layout, int cout, int cin, int ks) {
    if (cout <= 0 || cin <= 0 || cout > 4096 || cin > 4096) return 0;
    switch (layout) {
    case FG_EDM_PACK_GENERIC:
        if ((dtype != FG_DTYPE_F32 && dtype != FG_DTYPE_BF16 && dtype != FG_DTYPE_BF16X3) || (ks != 1 && ks != 3)) return 0;
        if ((cout % 32) || (cin % (dtype == FG_DTYPE_BF16 ? 64 : 32))) return 0;
        return conv_pack_elems(cout, cin, ks) * (dtype == FG_DTYPE_BF16 ? 2 : 4);
    case FG_EDM_PACK_WS:
        return dtype == FG_DTYPE_BF16 && ks == 3 && conv_ws_shape_ok(dtype, cout, cin, 32) ? conv_pack_elems(cout, cin, 3) * 2 : 0;
    case FG_EDM_PACK_X3WS:
        return dtype == FG_DTYPE_BF16X3 && ks == 3 && conv_x3ws_shape_ok(cout, cin, 32) ? conv_pack_elems(cout, cin, 3) * 4 : 0;
    case FG_EDM_PACK_X3SUB:
        return dtype == FG_DTYPE_BF16X3 && ks == 3 && conv_x3ws_shape_ok(cout, cin, 16) ? conv_pack_elems(cout, cin, 4) * 4 : 0;
    }
    return 0;
}

int fg_op_edm_conv_pack(int dtype, int layout, const float* w_oihw, void* packed, int cout, int cin, int ks, int qkv_perm, void* stream) {
    if (!fg_op_edm_conv_pack_bytes(dtype, layout, cout, cin, ks))
        return fail(FG_EINVAL, "fg_op_edm_conv_pack: no layout %d packing in dtype %d for cout %d, cin %d, ks %d", layout, dtype, cout, cin, ks);
    if (qkv_perm && (layout != FG_EDM_PACK_GENERIC || (cout % 3) || ks != 1))
        return fail(FG_EINVAL, "fg_op_edm_conv_pack: the q | k | v de-interleave belongs to the generic 1x1 layout with cout %d a multiple of 3", cout);
    if (!w_oihw || !packed) return fail(FG_EINVAL, "fg_op_edm_conv_pack: null pointer");
    if (!al16(packed)) return fail(FG_EINVAL, "fg_op_edm_conv_pack: packed must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    switch (layout) {
    case FG_EDM_PACK_GENERIC: HIP_TRY(launch_pack_conv_weights(dtype, w_oihw, packed, cout, cin, ks, qkv_perm ? 1 : 0, s)); break;
    case FG_EDM_PACK_WS: HIP_TRY(launch_pack_conv_weights_ws(w_oihw, packed, cout, cin, s)); break;
    case FG_EDM_PACK_X3WS: HIP_TRY(launch_pack_conv_weights_x3ws(w_oihw, packed, cout, cin, s)); break;
    default: HIP_TRY(launch_pack_conv_weights_x3sub(w_oihw, packed, cout, cin, s)); break;
    }
    return FG_OK;
}

int fg_op_edm_conv_plan(int dtype, int ks, int pro, int res, int outmode, int c1, int c2, int batch, int hs, int h, int cout, int has_wpack_ws,
                        int rshift, fg_edm_conv_plan* plan) {
    if (!plan) return fail(FG_EINVAL, "fg_op_edm_conv_plan: null plan");
    plan->kernel = 0, plan->stat_slots = 0;
    ConvArgs a{};
    if (const char* why = edm_conv_shape(dtype, ks, pro, res, outmode, c1, c2, batch, hs, h, cout, rshift, a))
        return fail(FG_EINVAL, "fg_op_edm_conv_plan: %s", why);
    // the predicates look at which operands exist, never through them
    static const float2 some{};
    a.ab = pro != PRO_NONE ? &some : nullptr;
    a.wpack = &some;
    a.wpack_ws = has_wpack_ws ? &some : nullptr;
    a.resid = rshift ? &some : nullptr;
    plan->kernel = edm_conv_kernel(dtype, ks, pro, res, outmode, a, &plan->stat_slots);
    if (!plan->kernel)
        return fail(FG_EINVAL, "fg_op_edm_conv_plan: no kernel for ks %d, pro %d, res %d, outmode %d, rshift %d in dtype %d at %dx%d (wave-specialised weights %s)",
                    ks, pro, res, outmode, rshift, dtype, h, h, has_wpack_ws ? "given" : "absent");
    return FG_OK;
}

int fg_op_edm_conv(int dtype, int ks, int pro, int res, int outmode, const void* src1, int c1, const void* src2, int c2, int batch, int hs, int h,
                   const float* ab, const void* wpack, const void* wpack_ws, const float* bias, const float* temb, int temb_stride, const void* resid,
                   int rshift, float scale, void* out, int cout, float* stats, void* q_out, void* k_out, void* vt_out, void* stream) {
    ConvArgs a{};
    if (const char* why = edm_conv_shape(dtype, ks, pro, res, outmode, c1, c2, batch, hs, h, cout, rshift, a)) return fail(FG_EINVAL, "fg_op_edm_conv: %s", why);
    if (!std::isfinite(scale)) return fail(FG_EINVAL, "fg_op_edm_conv: scale must be finite");
    if (!src1 || (c2 && !src2) || !wpack) return fail(FG_EINVAL, "fg_op_edm_conv: null src1 / src2 / wpack");
    if (pro != PRO_NONE && !ab) return fail(FG_EINVAL, "fg_op_edm_conv: pro %d needs the coefficients ab", pro);
    if (outmode == OUT_NHWC) {
        if (!out || q_out || k_out || vt_out) return fail(FG_EINVAL, "fg_op_edm_conv: the NHWC form writes out alone");
        if (temb && (temb_stride < cout || (temb_stride % 4))) return fail(FG_EINVAL, "fg_op_edm_conv: temb_stride %d must be a multiple of 4, at least cout %d", temb_stride, cout);
        if (rshift && !resid) return fail(FG_EINVAL, "fg_op_edm_conv: rshift without a residual");
    } else {
        if (out || temb || resid || stats || rshift) return fail(FG_EINVAL, "fg_op_edm_conv: the plane forms take no out, temb, resid, rshift or stats");
        if (!q_out || !vt_out || (outmode == OUT_QKV) != (k_out != nullptr)) return fail(FG_EINVAL, "fg_op_edm_conv: q_out, vt_out (and k_out of the q | k | v^T form alone)");
        if (scale != 1.0f) return fail(FG_EINVAL, "fg_op_edm_conv: the v^T plane is stored unscaled: scale must be 1");
    }
    if (!al16(src1) || !al16(src2) || !al16(wpack) || !al16(wpack_ws) || !al16(ab) || !al16(bias) || !al16(temb) || !al16(resid) || !al16(out) ||
        !al16(q_out) || !al16(k_out) || !al16(vt_out) || !al8(stats))
        return fail(FG_EINVAL, "fg_op_edm_conv: tensors, weights, ab, bias and temb must be 16-byte aligned, stats 8-byte aligned");
    a.src1 = src1, a.src2 = c2 ? src2 : nullptr, a.ab = pro != PRO_NONE ? (const float2*)ab : nullptr;
    a.wpack = wpack, a.wpack_ws = wpack_ws, a.bias = bias, a.temb = temb, a.temb_stride = temb_stride, a.resid = resid;
    a.scale = scale, a.out = out, a.stats = (float2*)stats, a.q_out = q_out, a.k_out = k_out, a.vt_out = vt_out;
    if (!edm_conv_kernel(dtype, ks, pro, res, outmode, a, nullptr))
        return fail(FG_EINVAL, "fg_op_edm_conv: no kernel for ks %d, pro %d, res %d, outmode %d, rshift %d in dtype %d at %dx%d (wave-specialised weights %s)", ks,
                    pro, res, outmode, rshift, dtype, h, h, wpack_ws ? "given" : "absent");
    static bool prepared[3][16] = {};  // the dynamic-LDS attributes, once per dtype and device
    const int dev = fg_device_slot();
    if (dev < 0) return fail(FG_EHIP, "fg_op_edm_conv: no current device");
    if (!prepared[dtype][dev]) {
        if (conv_prepare_all(dtype) != 0) return fail(FG_EHIP, "hipFuncSetAttribute(dynamic LDS) failed");
        prepared[dtype][dev] = true;
    }
    HIP_TRY(launch_conv_fused(dtype, ks, pro, res, outmode, a, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_edm_gn_finalize(const float* st1, int c1, int s1, const float* st2, int c2, int s2, const float* gamma, const float* beta, float eps,
                          float* ab, float* mr, int batch, int hw, void* stream) {
    if (!edm_gn_ok(c1, c2))
        return fail(FG_EINVAL, "fg_op_edm_gn_finalize: c1 %d > 0, c2 %d >= 0 multiples of 4, 16 <= c1 + c2 <= 512, groups of a multiple of 4 channels", c1, c2);
    if (s1 <= 0 || s1 > 4096 || (c2 && (s2 <= 0 || s2 > 4096))) return fail(FG_EINVAL, "fg_op_edm_gn_finalize: slot counts s1 %d, s2 %d must be 1 .. 4096", s1, s2);
    if (batch <= 0 || batch > 65535 || hw <= 0 || hw > (1 << 22)) return fail(FG_EINVAL, "fg_op_edm_gn_finalize: batch %d (1 .. 65535), hw %d (1 .. 2^22)", batch, hw);
    if (!(eps >= 0.f) || !std::isfinite(eps)) return fail(FG_EINVAL, "fg_op_edm_gn_finalize: eps must be finite and >= 0");
    if (!st1 || (c2 && !st2) || !gamma || !beta || !ab) return fail(FG_EINVAL, "fg_op_edm_gn_finalize: null pointer");
    if (!al8(st1) || !al8(st2) || !al8(ab) || !al8(mr)) return fail(FG_EINVAL, "fg_op_edm_gn_finalize: st1 / st2 / ab / mr must be 8-byte aligned");
    HIP_TRY(launch_gn_finalize((const float2*)st1, c1, s1, c2 ? (const float2*)st2 : nullptr, c2, c2 ? s2 : 0, gamma, beta, eps, (float2*)ab, batch, hw,
                               (hipStream_t)stream, (float2*)mr));
    return FG_OK;
}

int fg_op_edm_gn_silu_pool(int dtype, const void* x, const float* ab, void* out, int batch, int res_out, int c, void* stream) {
    if (dtype != FG_DTYPE_F32 && dtype != FG_DTYPE_BF16 && dtype != FG_DTYPE_BF16X3) return fail(FG_EINVAL, "fg_op_edm_gn_silu_pool: dtype %d (0, 1, 2)", dtype);
    if (c <= 0 || (c % 8) || c > 4096 || batch <= 0 || batch > 65535 || res_out <= 0 || res_out > 512)
        return fail(FG_EINVAL, "fg_op_edm_gn_silu_pool: c %d (a multiple of 8 up to 4096), batch %d (1 .. 65535), res_out %d (1 .. 512)", c, batch, res_out);
    if (!x || !ab || !out) return fail(FG_EINVAL, "fg_op_edm_gn_silu_pool: null pointer");
    if (!al16(x) || !al16(out) || !al8(ab)) return fail(FG_EINVAL, "fg_op_edm_gn_silu_pool: x / out must be 16-byte aligned, ab 8-byte aligned");
    HIP_TRY(launch_gn_silu_pool(edm_storage(dtype), x, (const float2*)ab, out, batch, res_out, res_out, c, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_edm_attention(int dtype, const void* q, const void* k, const void* vt, void* out, int batch, int t, void* stream) {
    if (dtype != FG_DTYPE_F32 && dtype != FG_DTYPE_BF16 && dtype != FG_DTYPE_BF16X3) return fail(FG_EINVAL, "fg_op_edm_attention: dtype %d (0, 1, 2)", dtype);
    if ((t != 64 && t != 256) || batch <= 0 || batch > 65535) return fail(FG_EINVAL, "fg_op_edm_attention: t %d (64, 256), batch %d (1 .. 65535)", t, batch);
    if (!q || !k || !vt || !out) return fail(FG_EINVAL, "fg_op_edm_attention: null pointer");
    if (!al16(q) || !al16(k) || !al16(vt) || !al16(out)) return fail(FG_EINVAL, "fg_op_edm_attention: tensors must be 16-byte aligned");
    HIP_TRY(launch_attention(dtype, q, k, vt, out, batch, t, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_edm_attn_merge_weights(const float* qkv_w, const float* qkv_b, const float* proj_w, float* w_out, float* b_out, int c, void* stream) {
    if (c <= 0 || c > 4096) return fail(FG_EINVAL, "fg_op_edm_attn_merge_weights: c %d (1 .. 4096)", c);
    if (!qkv_w || !qkv_b || !proj_w || !w_out || !b_out) return fail(FG_EINVAL, "fg_op_edm_attn_merge_weights: null pointer");
    HIP_TRY(launch_attn_merge_weights(qkv_w, qkv_b, proj_w, w_out, b_out, c, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_edm_attention_merged(const float* qm, const float* x_mid, const float* ab, const float* vmt, const float* bp, float scale, float* out,
                               float* stats, int batch, void* stream) {
    if (batch <= 0 || batch > 32767) return fail(FG_EINVAL, "fg_op_edm_attention_merged: batch %d (1 .. 32767)", batch);
    if (!std::isfinite(scale)) return fail(FG_EINVAL, "fg_op_edm_attention_merged: scale must be finite");
    if (!qm || !x_mid || !ab || !vmt || !bp || !out) return fail(FG_EINVAL, "fg_op_edm_attention_merged: null pointer");
    if (!al16(qm) || !al16(x_mid) || !al16(ab) || !al16(vmt) || !al16(bp) || !al16(out) || !al8(stats))
        return fail(FG_EINVAL, "fg_op_edm_attention_merged: tensors, ab and bp must be 16-byte aligned, stats 8-byte aligned");
    HIP_TRY(launch_attention_merged(qm, x_mid, (const float2*)ab, vmt, bp, scale, out, (float2*)stats, batch, (hipStream_t)stream));
    return FG_OK;
}

size_t fg_op_edm_head_pack_bytes(int which, int dtype, int c) {
    if (dtype != FG_DTYPE_F32 && dtype != FG_DTYPE_BF16 && dtype != FG_DTYPE_BF16X3) return 0;
    if (which == FG_EDM_PACK_STEM) return stem_pack_elems() * (edm_storage(dtype) ? 2 : 4);
    if (which == FG_EDM_PACK_AUX) return c > 0 && c <= 4096 && !(c % (dtype == FG_DTYPE_BF16 ? 64 : 32)) ? aux_pack_elems(c) * (dtype == FG_DTYPE_BF16 ? 2 : 4) : 0;
    return 0;
}

int fg_op_edm_stem(int dtype, const float* x, const float* coef, const float* w_oihw, void* packed, const float* bias, void* out, float* stats, int batch,
                   int res, int cin, void* stream) {
    if (dtype != FG_DTYPE_F32 && dtype != FG_DTYPE_BF16 && dtype != FG_DTYPE_BF16X3) return fail(FG_EINVAL, "fg_op_edm_stem: dtype %d (0, 1, 2)", dtype);
    if (cin <= 0 || res <= 0 || res > 1024 || !stem_supported(res, cin, 128))
        return fail(FG_EINVAL, "fg_op_edm_stem: cin %d (9 cin <= 32), res %d (res^2 a multiple of 32, up to 1024)", cin, res);
    if (batch <= 0 || batch > 65535) return fail(FG_EINVAL, "fg_op_edm_stem: batch %d (1 .. 65535)", batch);
    if (!x || !coef || !w_oihw || !packed || !bias || !out) return fail(FG_EINVAL, "fg_op_edm_stem: null pointer");
    if (!al16(packed) || !al16(out) || !al8(stats)) return fail(FG_EINVAL, "fg_op_edm_stem: packed / out must be 16-byte aligned, stats 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int st = edm_storage(dtype);
    HIP_TRY(launch_pack_stem_weights(st, w_oihw, packed, cin, s));
    HIP_TRY(launch_stem(st, x, coef, packed, bias, out, (float2*)stats, batch, res, cin, s));
    return FG_OK;
}

int fg_op_edm_conv_in(int dtype, const float* x, const float* coef, const float* w_oihw, const float* bias, void* out, int batch, int res, int cin, int cout,
                      void* stream) {
    if (dtype != FG_DTYPE_F32 && dtype != FG_DTYPE_BF16 && dtype != FG_DTYPE_BF16X3) return fail(FG_EINVAL, "fg_op_edm_conv_in: dtype %d (0, 1, 2)", dtype);
    if (cin <= 0 || cout <= 0 || (cout % 16) || (size_t)cin * 9 * cout * sizeof(float) > 64 * 1024)
        return fail(FG_EINVAL, "fg_op_edm_conv_in: cin %d > 0, cout %d a multiple of 16, 36 cin cout <= 65536 bytes of LDS", cin, cout);
    if (batch <= 0 || res <= 0 || res > 1024 || (int64_t)batch * res > (1 << 30)) return fail(FG_EINVAL, "fg_op_edm_conv_in: batch %d, res %d (1 .. 1024)", batch, res);
    if (!x || !coef || !w_oihw || !bias || !out) return fail(FG_EINVAL, "fg_op_edm_conv_in: null pointer");
    if (!al16(out)) return fail(FG_EINVAL, "fg_op_edm_conv_in: out must be 16-byte aligned");
    HIP_TRY(launch_conv_in(edm_storage(dtype), x, coef, w_oihw, bias, out, batch, res, cin, cout, (hipStream_t)stream));
    return FG_OK;
}

int fg_op_edm_aux_head(int dtype, const void* x, const float* ab, const float* w_oihw, void* packed, const float* bias, const float* x_t, const float* coef,
                       float* out, int batch, int c, int cout, void* stream) {
    if (dtype != FG_DTYPE_F32 && dtype != FG_DTYPE_BF16 && dtype != FG_DTYPE_BF16X3) return fail(FG_EINVAL, "fg_op_edm_aux_head: dtype %d (0, 1, 2)", dtype);
    if (c <= 0 || c > 4096 || cout <= 0 || !aux_head_supported(dtype, 32, c, cout))
        return fail(FG_EINVAL, "fg_op_edm_aux_head: c %d (a multiple of the K step: 64 in bf16, else 32), cout %d (1 .. 32)", c, cout);
    if (batch <= 0 || batch > 65535) return fail(FG_EINVAL, "fg_op_edm_aux_head: batch %d (1 .. 65535)", batch);
    if (!x || !ab || !w_oihw || !packed || !bias || !x_t || !coef || !out) return fail(FG_EINVAL, "fg_op_edm_aux_head: null pointer");
    if (!al16(x) || !al16(ab) || !al16(packed)) return fail(FG_EINVAL, "fg_op_edm_aux_head: x / ab / packed must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_pack_aux_weights(dtype, w_oihw, packed, c, cout, s));
    HIP_TRY(launch_aux_head(dtype, x, (const float2*)ab, packed, bias, x_t, coef, out, batch, c, cout, s));
    return FG_OK;
}

int fg_op_edm_aux_out(int dtype, const void* x, const float* ab, const float* w_oihw, const float* bias, const float* x_t, const float* coef, float* out,
                      int batch, int res, int c, int cout, void* stream) {
    if (dtype != FG_DTYPE_F32 && dtype != FG_DTYPE_BF16 && dtype != FG_DTYPE_BF16X3) return fail(FG_EINVAL, "fg_op_edm_aux_out: dtype %d (0, 1, 2)", dtype);
    if (c <= 0 || (c % 32) || cout <= 0 || cout > 4 || (size_t)9 * cout * c * sizeof(float) + (size_t)c * sizeof(float2) > 64 * 1024)
        return fail(FG_EINVAL, "fg_op_edm_aux_out: c %d (a multiple of 32), cout %d (1 .. 4), 36 cout c + 8 c <= 65536 bytes of LDS", c, cout);
    if (batch <= 0 || res <= 0 || res > 1024 || (int64_t)batch * res > (1 << 30)) return fail(FG_EINVAL, "fg_op_edm_aux_out: batch %d, res %d (1 .. 1024)", batch, res);
    if (!x || !ab || !w_oihw || !bias || !x_t || !coef || !out) return fail(FG_EINVAL, "fg_op_edm_aux_out: null pointer");
    if (!al16(x) || !al8(ab)) return fail(FG_EINVAL, "fg_op_edm_aux_out: x must be 16-byte aligned, ab 8-byte aligned");
    HIP_TRY(launch_aux_out(edm_storage(dtype), x, (const float2*)ab, w_oihw, bias, x_t, coef, out, batch, res, c, cout, (hipStream_t)stream, nullptr));
    return FG_OK;
}
