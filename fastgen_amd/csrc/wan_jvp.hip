// Forward-mode derivative (jvp) of the bidirectional video DiT (Wan/network.py through engine_wan_jvp.inc): the pieces that are not
// GEMMs, each carrying a tangent beside its primal.  Token tensors are bf16 in both streams, statistics / softmax / modulation rows
// fp32, as in wan.hip.  Every kernel is mirrored in fp64 by tests/wan_jvp_ref.py.
//   wan_ln_modulate_jvp_kernel  n = LN(x), y = n (1 + s) + b;  nd = (xd - mean(xd) - n mean(n xd)) / sigma, yd = nd (1 + s) + n sd + bd
//   wan_rms_rope_jvp_kernel     n = x / rms, nd = (xd - n mean(n xd)) / rms, both times w, then the same pair rotation (RoPE is linear)
//   wan_attn_jvp_kernel         softmax(q k^T / sqrt(128)) v with tangent, flash form, any number of keys
//   wan_gelu_jvp_kernel         a = gelu_tanh(h), ad = gelu_tanh'(h) hd
//   wan_final_jvp_kernel        wan_final_kernel with the tangent of the LayerNorm-modulate: out = b + W y, jvp = W yd
//   wan_dup2_kernel             the output layer's {shift, scale} tangent rows: both are the tangent of temb
#include "common.h"
#include "misc.h"

namespace {

typedef __attribute__((ext_vector_type(2))) __bf16 wj_bf16x2;

__device__ __forceinline__ float wj_wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One wave per token, D = 128 NP, lane l holds the channel pairs 2 (l + 64 j).  mod / modd [rows][mod_stride] fp32: shift at shift_off,
// scale at scale_off, their tangents at the same places of modd (modd == nullptr: a constant affine, sd = bd = 0); row = tok / tpi.
template <int NP>
__global__ __launch_bounds__(256) void wan_ln_modulate_jvp_kernel(const __bf16* __restrict__ x, const __bf16* __restrict__ xd,
                                                                  const float* __restrict__ mod, const float* __restrict__ modd, int mod_stride,
                                                                  int shift_off, int scale_off, __bf16* __restrict__ y, __bf16* __restrict__ yd,
                                                                  int ntok, int tpi, float eps) {
    constexpr int D = 128 * NP;
    const int lane = threadIdx.x & 63;
    const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= ntok) return;
    const int n = tok / tpi;
    float v[2 * NP], d[2 * NP];
    float s = 0.f, sd = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const wj_bf16x2 q = *reinterpret_cast<const wj_bf16x2*>(x + (size_t)tok * D + 2 * (lane + 64 * j));
        const wj_bf16x2 p = *reinterpret_cast<const wj_bf16x2*>(xd + (size_t)tok * D + 2 * (lane + 64 * j));
        v[2 * j] = (float)q[0], v[2 * j + 1] = (float)q[1], d[2 * j] = (float)p[0], d[2 * j + 1] = (float)p[1];
        s += v[2 * j] + v[2 * j + 1];
        sd += d[2 * j] + d[2 * j + 1];
    }
    const float mean = wj_wsum(s) * (1.0f / D), dmean = wj_wsum(sd) * (1.0f / D);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 2 * NP; ++e) {
        v[e] -= mean;
        ss = fmaf(v[e], v[e], ss);
    }
    const float rstd = 1.0f / sqrtf(wj_wsum(ss) * (1.0f / D) + eps);
    float nd = 0.f;
#pragma unroll
    for (int e = 0; e < 2 * NP; ++e) {
        v[e] *= rstd;
        nd = fmaf(v[e], d[e], nd);
    }
    const float m2 = wj_wsum(nd) * (1.0f / D);
    const float* mrow = mod + (size_t)n * mod_stride;
    const float* mdrow = modd ? modd + (size_t)n * mod_stride : nullptr;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int c = 2 * (lane + 64 * j);
        const f32x2 sc = *reinterpret_cast<const f32x2*>(mrow + scale_off + c), sh = *reinterpret_cast<const f32x2*>(mrow + shift_off + c);
        f32x2 scd = {0.f, 0.f}, shd = {0.f, 0.f};
        if (mdrow) scd = *reinterpret_cast<const f32x2*>(mdrow + scale_off + c), shd = *reinterpret_cast<const f32x2*>(mdrow + shift_off + c);
        float o[2], od[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float nn = v[2 * j + e], ndv = (d[2 * j + e] - dmean - nn * m2) * rstd;
            o[e] = fmaf(nn, 1.0f + sc[e], sh[e]);
            od[e] = fmaf(ndv, 1.0f + sc[e], fmaf(nn, scd[e], shd[e]));
        }
        *reinterpret_cast<wj_bf16x2*>(y + (size_t)tok * D + c) = wj_bf16x2{(__bf16)o[0], (__bf16)o[1]};
        *reinterpret_cast<wj_bf16x2*>(yd + (size_t)tok * D + c) = wj_bf16x2{(__bf16)od[0], (__bf16)od[1]};
    }
}

// rms_rope_kernel of wan.hip with a tangent: one wave per row, rows of src / srcd [rows][ld_src], w != nullptr; cs nullable (no
// rotation); row r = (batch r / L, token r % L) goes to dst / dstd + batch * dst_bs + token * ld_dst.
template <int NP>
__global__ __launch_bounds__(256) void wan_rms_rope_jvp_kernel(const __bf16* __restrict__ src, const __bf16* __restrict__ srcd, int ld_src,
                                                               const float* __restrict__ w, float eps, const float2* __restrict__ cs,
                                                               __bf16* __restrict__ dst, __bf16* __restrict__ dstd, int64_t dst_bs, int ld_dst,
                                                               int rows, int L) {
    constexpr int D = 128 * NP;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[2 * NP], d[2 * NP];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const wj_bf16x2 q = *reinterpret_cast<const wj_bf16x2*>(src + (size_t)row * ld_src + 2 * (lane + 64 * j));
        const wj_bf16x2 p = *reinterpret_cast<const wj_bf16x2*>(srcd + (size_t)row * ld_src + 2 * (lane + 64 * j));
        v[2 * j] = (float)q[0], v[2 * j + 1] = (float)q[1], d[2 * j] = (float)p[0], d[2 * j + 1] = (float)p[1];
        ss = fmaf(v[2 * j], v[2 * j], fmaf(v[2 * j + 1], v[2 * j + 1], ss));
    }
    const float r = 1.0f / sqrtf(wj_wsum(ss) * (1.0f / D) + eps);
    float nd = 0.f;
#pragma unroll
    for (int e = 0; e < 2 * NP; ++e) {
        v[e] *= r;
        nd = fmaf(v[e], d[e], nd);
    }
    const float m2 = wj_wsum(nd) * (1.0f / D);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const f32x2 wq = *reinterpret_cast<const f32x2*>(w + 2 * (lane + 64 * j));
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            d[2 * j + e] = (d[2 * j + e] - v[2 * j + e] * m2) * r * wq[e];
            v[2 * j + e] *= wq[e];
        }
    }
    const int b = row / L, l = row - b * L;
    if (cs) {
        const float2 c = cs[(size_t)l * 64 + lane];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const float a = v[2 * j], bb = v[2 * j + 1], ad = d[2 * j], bd = d[2 * j + 1];
            v[2 * j] = a * c.x - bb * c.y;
            v[2 * j + 1] = a * c.y + bb * c.x;
            d[2 * j] = ad * c.x - bd * c.y;
            d[2 * j + 1] = ad * c.y + bd * c.x;
        }
    }
    const size_t at = (size_t)b * dst_bs + (size_t)l * ld_dst;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        *reinterpret_cast<wj_bf16x2*>(dst + at + 2 * (lane + 64 * j)) = wj_bf16x2{(__bf16)v[2 * j], (__bf16)v[2 * j + 1]};
        *reinterpret_cast<wj_bf16x2*>(dstd + at + 2 * (lane + 64 * j)) = wj_bf16x2{(__bf16)d[2 * j], (__bf16)d[2 * j + 1]};
    }
}

// ---- attention with tangent, head dim 128 ---------------------------------------------------------------------------------------
//   S = q k^T / sqrt(hd), P = softmax(S), O = P v
//   Sd = (qd k^T + q kd^T) / sqrt(hd), delta_i = sum_j P_ij Sd_ij, Od = (P o (Sd - delta)) v + P vd
// delta_i is known only after the last key, so the kernel carries, for a per-query reference c_i fixed at the first key tile,
//   W_ij = P_ij (Sd_ij - c_i),   T = sum_j (W_ij v_j + P_ij vd_j),   w = sum_j W_ij,   l = sum_j P_ij,   O~ = sum_j P_ij v_j
// with P un-normalised (2^(scale (S - m))); all four take the online-softmax rescale, and at the end
//   O_i = O~ / l,   Od_i = T / l - (w / l) O_i                                  (exact for every c_i: dit_jvp.hip's identity)
// c_i = the mean of Sd over the first key tile: what is common to a row of Sd (the shift tangent of the modulation reaches every key
// of a frame alike and is the largest part of kd under the x1000 timestep scale) leaves before W is rounded to bf16.
// Layout as wan.hip's fa_kernel<128> in its register-staged form: grid = (sample, head) units dealt to the XCDs x query tiles of 128,
// a wave owns 32 queries; S^T = K Q^T and Sd^T = K Qd^T + Kd Q^T put the query on the lane (softmax state, c, w, l: one lane's
// scalars), P^T and W^T are the B operands of O~^T = V^T P^T and T^T = V^T W^T + Vd^T P^T: five products per key tile.  The K, V,
// Kd, Vd tiles of 32 keys (8 KiB each, fa_kernel's swizzled image) are double-buffered in 64 KiB of LDS; the next tile's rows are in
// flight in registers while a tile is computed.  Key rows are clamped to Lkv - 1 when loaded (nothing past the last key is read) and
// masked in S.  Null qd / kd / vd: that tangent is zero and its product is skipped (the text keys of the cross-attention).
__device__ __forceinline__ int wj_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }
typedef __attribute__((ext_vector_type(4))) short wj_s16x4;
typedef __attribute__((ext_vector_type(8))) short wj_s16x8;
typedef __attribute__((address_space(3))) wj_s16x4 wj_lds_s16x4;
__device__ __forceinline__ wj_s16x4 wj_tr_read(const char* lds_addr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((wj_lds_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)lds_addr);
}
// the value of the other lane half (lane ^ 32) combined with this one's
__device__ __forceinline__ void wj_swap(float v, float& a_, float& b_) {
    a_ = v, b_ = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a_), "+v"(b_));
}

__global__ __launch_bounds__(256, 1) void wan_attn_jvp_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ qd, int ldq, int64_t q_bs,
                                                              const __bf16* __restrict__ k, const __bf16* __restrict__ v,
                                                              const __bf16* __restrict__ kd, const __bf16* __restrict__ vd, int ldk,
                                                              int64_t kv_bs, __bf16* __restrict__ out, __bf16* __restrict__ outd, int ldo,
                                                              int64_t o_bs, int Lq, int Lkv, float scale, int heads, int batch) {
    constexpr int HD = 128, KS = 8, DT_ = 4, TILE = 32 * 256, BUF = 4 * TILE;  // a buffer = K | V | Kd | Vd tiles
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int qtiles = (Lq + 127) / 128, units = batch * heads;
    const int xcd = (int)blockIdx.x & 7, slot = (int)blockIdx.x >> 3;
    const int qt = slot % qtiles, unit = (slot / qtiles) * 8 + xcd;
    if (unit >= units) return;  // (the grid is padded to a multiple of 8 units; uniform per workgroup, before any barrier)
    const int head = unit % heads, b = unit / heads;
    const int q0 = qt * 128 + wave * 32;
    const float scale_log2e = scale * 1.44269504088896341f;
    // this lane's query row (clamped: rows past Lq compute on the last row and are not stored)
    const size_t qat = (size_t)b * q_bs + (size_t)min(q0 + r, Lq - 1) * ldq + head * HD + 8 * h;
    bf16x8 qf[KS], qdf[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
        qf[kk] = *reinterpret_cast<const bf16x8*>(q + qat + kk * 16);
        qdf[kk] = bf16x8{};
        if (qd) qdf[kk] = *reinterpret_cast<const bf16x8*>(qd + qat + kk * 16);
    }
    const size_t kvat = (size_t)b * kv_bs + head * HD;
    // staging: 32 rows x 16 chunks of 16 bytes per tile over 256 threads = 2 chunks per thread and tile
    fg_u32x4 kreg[2], vreg[2], kdreg[2], vdreg[2];
    auto issue = [&](int t) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = tid + 256 * i;
            const size_t at = kvat + (size_t)min(t * 32 + (p >> 4), Lkv - 1) * ldk + (p & 15) * 8;
            kreg[i] = *reinterpret_cast<const fg_u32x4*>(k + at);
            vreg[i] = *reinterpret_cast<const fg_u32x4*>(v + at);
            if (kd) kdreg[i] = *reinterpret_cast<const fg_u32x4*>(kd + at);
            if (vd) vdreg[i] = *reinterpret_cast<const fg_u32x4*>(vd + at);
        }
    };
    auto park = [&](char* st) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = tid + 256 * i, o = wj_off(p >> 4, p & 15);
            *reinterpret_cast<fg_u32x4*>(st + o) = kreg[i];
            *reinterpret_cast<fg_u32x4*>(st + TILE + o) = vreg[i];
            if (kd) *reinterpret_cast<fg_u32x4*>(st + 2 * TILE + o) = kdreg[i];
            if (vd) *reinterpret_cast<fg_u32x4*>(st + 3 * TILE + o) = vdreg[i];
        }
    };
    f32x16 ot[DT_], tt[DT_];
#pragma unroll
    for (int d = 0; d < DT_; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) ot[d][i] = 0.f, tt[d][i] = 0.f;
    float m = -INFINITY, lsum = 0.f, wsum = 0.f, cref = 0.f;  // (lsum, wsum: this lane's half of the query's keys; the halves meet in the epilogue)
    // transposed-read lane addresses inside a V tile, as fa_kernel
    const int gi = lane & 15, gq = gi >> 2, gp = gi & 3, gc = (lane >> 4) & 1;
    const int ntiles = (Lkv + 31) / 32;
    issue(0);
    park(smem);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const char* st = smem + (t & 1) * BUF;
        if (t + 1 < ntiles) issue(t + 1);
        // S^T[key][query] and Sd^T
        f32x16 s, sd;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f, sd[i] = 0.f;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(st + wj_off(r, 2 * kk + h));
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], s, 0, 0, 0);
            if (qd) sd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qdf[kk], sd, 0, 0, 0);
        }
        if (kd) {
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const bf16x8 kdf = *reinterpret_cast<const bf16x8*>(st + 2 * TILE + wj_off(r, 2 * kk + h));
                sd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kdf, qf[kk], sd, 0, 0, 0);
            }
        }
        if (t == ntiles - 1) {  // (wave-uniform) only the last key tile can be ragged
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (t * 32 + acc_row(i, h) >= Lkv) s[i] = -INFINITY;
        }
        float a_, b_;
        if (t == 0) {  // the reference: the mean of Sd over the first tile (clamped rows repeat the last key: any c_i is exact)
            float c = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) c += sd[i];
            wj_swap(c, a_, b_);
            cref = (a_ + b_) * scale * (1.0f / 32.0f);
        }
        float mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) mt = fmaxf(mt, s[i]);
        wj_swap(mt, a_, b_);
        mt = fmaxf(a_, b_);
        const float mn = fmaxf(m, mt);
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale_log2e);  // m = -inf at the first tile: exp2(-inf) = 0
        const float mc = mn * scale_log2e;
        m = mn;
        float e[16], wv[16];
        float ps = 0.f, pw = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            e[i] = __builtin_amdgcn_exp2f(fmaf(s[i], scale_log2e, -mc));
            wv[i] = e[i] * fmaf(sd[i], scale, -cref);
            ps += e[i];
            pw += wv[i];
        }
        lsum = fmaf(lsum, alpha, ps);
        wsum = fmaf(wsum, alpha, pw);
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {  // wave-uniform: the running maximum of some query of this wave moved
#pragma unroll
            for (int d = 0; d < DT_; ++d)
#pragma unroll
                for (int i = 0; i < 16; ++i) ot[d][i] *= alpha, tt[d][i] *= alpha;
        }
        // O~^T[dim][query] += V^T P^T;  T^T += V^T W^T + Vd^T P^T
#pragma unroll
        for (int sx = 0; sx < 2; ++sx) {
            bf16x8 pf, wf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (__bf16)e[8 * sx + j], wf[j] = (__bf16)wv[8 * sx + j];
#pragma unroll
            for (int d = 0; d < DT_; ++d) {
                const int r0 = 16 * sx + 4 * h, c0 = 4 * d + 2 * gc;
                const int olo = wj_off(r0 + gq, c0 + (gp >> 1)) + 8 * (gp & 1), ohi = wj_off(r0 + 8 + gq, c0 + (gp >> 1)) + 8 * (gp & 1);
                const wj_s16x4 lo = wj_tr_read(st + TILE + olo), hi = wj_tr_read(st + TILE + ohi);
                const bf16x8 vv = __builtin_bit_cast(bf16x8, wj_s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
                ot[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vv, pf, ot[d], 0, 0, 0);
                tt[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vv, wf, tt[d], 0, 0, 0);
                if (vd) {
                    const wj_s16x4 dl = wj_tr_read(st + 3 * TILE + olo), dh = wj_tr_read(st + 3 * TILE + ohi);
                    const bf16x8 dv = __builtin_bit_cast(bf16x8, wj_s16x8{dl[0], dl[1], dl[2], dl[3], dh[0], dh[1], dh[2], dh[3]});
                    tt[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dv, pf, tt[d], 0, 0, 0);
                }
            }
        }
        if (t + 1 < ntiles) park(smem + ((t + 1) & 1) * BUF);  // (its last readers passed the barrier that ended tile t - 1)
        __syncthreads();
    }
    float a_, b_;
    wj_swap(lsum, a_, b_);
    lsum = a_ + b_;
    wj_swap(wsum, a_, b_);
    wsum = a_ + b_;
    // out / outd[query][head * HD + dim]: this lane holds dims 32 d + 8 i4 + 4 h + e of its query
    if (q0 + r < Lq) {
        const float inv = 1.0f / lsum, wn = wsum * inv;
        const size_t at = (size_t)b * o_bs + (size_t)(q0 + r) * ldo + head * HD;
#pragma unroll
        for (int d = 0; d < DT_; ++d)
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) {
                bf16x4 o4, d4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float o = ot[d][4 * i4 + e] * inv;
                    o4[e] = (__bf16)o;
                    d4[e] = (__bf16)fmaf(-wn, o, tt[d][4 * i4 + e] * inv);
                }
                *reinterpret_cast<bf16x4*>(out + at + 32 * d + 8 * i4 + 4 * h) = o4;
                *reinterpret_cast<bf16x4*>(outd + at + 32 * d + 8 * i4 + 4 * h) = d4;
            }
    }
}

// a = gelu_tanh(h) = h sig(2 u), u = sqrt(2/pi) (h + 0.044715 h^3);  ad = (sig + h sig (1 - sig) 2 u') hd (dit_jvp.hip's
// gelu_jvp_kernel on bf16 tensors).  h, hd, a, ad bf16 [n]; one thread = 4 values; a / ad may be h / hd (each thread reads its four
// values before it writes them).
__global__ __launch_bounds__(256) void wan_gelu_jvp_kernel(const __bf16* h, const __bf16* hd, __bf16* a, __bf16* ad, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const bf16x4 x = *reinterpret_cast<const bf16x4*>(h + 4 * i), xd = *reinterpret_cast<const bf16x4*>(hd + 4 * i);
    bf16x4 g4, gd4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        constexpr float c0 = 0.7978845608028654f, c1 = 0.044715f;
        const float v = (float)x[e], v2 = v * v;
        const float u2 = 2.0f * c0 * v * fmaf(c1, v2, 1.0f);
        const float sig = 1.0f / (1.0f + expf(-u2));
        const float g = v * sig;
        g4[e] = (__bf16)g;
        gd4[e] = (__bf16)((sig + g * (1.0f - sig) * (2.0f * c0 * fmaf(3.0f * c1, v2, 1.0f))) * (float)xd[e]);
    }
    *reinterpret_cast<bf16x4*>(a + 4 * i) = g4;
    *reinterpret_cast<bf16x4*>(ad + 4 * i) = gd4;
}

// modd[r][0][d] = modd[r][1][d] = tembd[r][d]: the tangent of the output layer's table + temb rows is temb's, for shift and scale alike
__global__ void wan_dup2_kernel(const float* __restrict__ tembd, float* __restrict__ modd, int rows, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * 2 * D) return;
    modd[i] = tembd[(i / (2 * (int64_t)D)) * D + i % D];
}

// wan_final_kernel of wan.hip with a tangent: mod / modd [B * Fr][2][D] = {shift, scale} and their tangents; out, outd [B][C][F][H][W]
template <int NP>
__global__ __launch_bounds__(256) void wan_final_jvp_kernel(const __bf16* __restrict__ x, const __bf16* __restrict__ xd,
                                                            const float* __restrict__ mod, const float* __restrict__ modd,
                                                            const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out,
                                                            float* __restrict__ outd, int ntok, int Fr, int gh, int gw, int C, float eps) {
    constexpr int D = 128 * NP;
    const int lane = threadIdx.x & 63;
    const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= ntok) return;
    const int fs = gh * gw;
    const int bf = tok / fs, hw = tok - bf * fs, b = bf / Fr, f = bf - b * Fr, gy = hw / gw, gx = hw - gy * gw;
    float v[2 * NP], d[2 * NP];
    float s = 0.f, sd = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const wj_bf16x2 q = *reinterpret_cast<const wj_bf16x2*>(x + (size_t)tok * D + 2 * (lane + 64 * j));
        const wj_bf16x2 p = *reinterpret_cast<const wj_bf16x2*>(xd + (size_t)tok * D + 2 * (lane + 64 * j));
        v[2 * j] = (float)q[0], v[2 * j + 1] = (float)q[1], d[2 * j] = (float)p[0], d[2 * j + 1] = (float)p[1];
        s += v[2 * j] + v[2 * j + 1];
        sd += d[2 * j] + d[2 * j + 1];
    }
    const float mean = wj_wsum(s) * (1.0f / D), dmean = wj_wsum(sd) * (1.0f / D);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 2 * NP; ++e) {
        v[e] -= mean;
        ss = fmaf(v[e], v[e], ss);
    }
    const float rstd = 1.0f / sqrtf(wj_wsum(ss) * (1.0f / D) + eps);
    float nd = 0.f;
#pragma unroll
    for (int e = 0; e < 2 * NP; ++e) {
        v[e] *= rstd;
        nd = fmaf(v[e], d[e], nd);
    }
    const float m2 = wj_wsum(nd) * (1.0f / D);
    const float *mrow = mod + (size_t)bf * 2 * D, *mdrow = modd + (size_t)bf * 2 * D;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int c = 2 * (lane + 64 * j);
        const f32x2 sh = *reinterpret_cast<const f32x2*>(mrow + c), sc = *reinterpret_cast<const f32x2*>(mrow + D + c);
        const f32x2 shd = *reinterpret_cast<const f32x2*>(mdrow + c), scd = *reinterpret_cast<const f32x2*>(mdrow + D + c);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float nn = v[2 * j + e], ndv = (d[2 * j + e] - dmean - nn * m2) * rstd;
            v[2 * j + e] = fmaf(nn, 1.0f + sc[e], sh[e]);
            d[2 * j + e] = fmaf(ndv, 1.0f + sc[e], fmaf(nn, scd[e], shd[e]));
        }
    }
    const int H = 2 * gh, W = 2 * gw;
    for (int o = 0; o < 4 * C; ++o) {
        float a = 0.f, ad = 0.f;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const f32x2 q = *reinterpret_cast<const f32x2*>(w + (size_t)o * D + 2 * (lane + 64 * j));
            a = fmaf(v[2 * j], q[0], a), a = fmaf(v[2 * j + 1], q[1], a);
            ad = fmaf(d[2 * j], q[0], ad), ad = fmaf(d[2 * j + 1], q[1], ad);
        }
        a = wj_wsum(a);
        ad = wj_wsum(ad);
        if (lane == 0) {
            const int c = o % C, pq = o / C, py = pq >> 1, px = pq & 1;
            const size_t at = ((((size_t)b * C + c) * Fr + f) * H + 2 * gy + py) * W + 2 * gx + px;
            out[at] = a + bias[o];
            outd[at] = ad;
        }
    }
}

#define WJ_RET() return (int)hipGetLastError()
// D = 128 NP with NP in {2, 3, 12, 16, 24, 40}, as wan.hip's launchers
#define WJ_SWITCH(D, GO)                           \
    switch (D) {                                   \
        case 256: GO(2); break;                    \
        case 384: GO(3); break;                    \
        case 1536: GO(12); break;                  \
        case 2048: GO(16); break;                  \
        case 3072: GO(24); break;                  \
        case 5120: GO(40); break;                  \
        default: return (int)hipErrorInvalidValue; \
    }

}  // namespace

int launch_wan_ln_modulate_jvp(int D, const void* x, const void* xd, const float* mod, const float* modd, int mod_stride, int shift_off,
                               int scale_off, void* y, void* yd, int ntok, int tokens_per_row, float eps, hipStream_t s) {
    if (ntok <= 0 || tokens_per_row <= 0 || (mod_stride % 2) || (shift_off % 2) || (scale_off % 2)) return (int)hipErrorInvalidValue;  // (8-byte loads)
    dim3 g((ntok + 3) / 4), b(256);
#define GO(NP)                                                                                                                                    \
    hipLaunchKernelGGL(wan_ln_modulate_jvp_kernel<NP>, g, b, 0, s, (const __bf16*)x, (const __bf16*)xd, mod, modd, mod_stride, shift_off, scale_off, \
                       (__bf16*)y, (__bf16*)yd, ntok, tokens_per_row, eps)
    WJ_SWITCH(D, GO)
#undef GO
    WJ_RET();
}
int launch_wan_rms_rope_jvp(int D, const void* src, const void* srcd, int ld_src, const float* w, float eps, const float2* cs, void* dst, void* dstd,
                            int64_t dst_bs, int ld_dst, int rows, int L, hipStream_t s) {
    if (rows <= 0 || L <= 0 || !w || (ld_src % 2) || (ld_dst % 2)) return (int)hipErrorInvalidValue;
    dim3 g((rows + 3) / 4), b(256);
#define GO(NP)                                                                                                                                  \
    hipLaunchKernelGGL(wan_rms_rope_jvp_kernel<NP>, g, b, 0, s, (const __bf16*)src, (const __bf16*)srcd, ld_src, w, eps, cs, (__bf16*)dst, (__bf16*)dstd, \
                       dst_bs, ld_dst, rows, L)
    WJ_SWITCH(D, GO)
#undef GO
    WJ_RET();
}
int launch_wan_attention_jvp(const void* q, const void* qd, int ldq, int64_t q_bs, const void* k, const void* v, const void* kd, const void* vd,
                             int ldk, int64_t kv_bs, void* out, void* outd, int ldo, int64_t o_bs, int B, int heads, int Lq, int Lkv,
                             hipStream_t s) {
    if (B <= 0 || heads <= 0 || Lq <= 0 || Lkv <= 0 || ldq <= 0 || ldk <= 0 || ldo <= 0 || (ldq % 8) || (ldk % 8) || (ldo % 4) || (q_bs % 8) ||
        (kv_bs % 8) || (o_bs % 4))  // (16-byte loads, 8-byte stores)
        return (int)hipErrorInvalidValue;
    const int64_t units = (int64_t)B * heads, grid = ((units + 7) / 8) * 8 * ((Lq + 127) / 128);
    if (grid > INT32_MAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(wan_attn_jvp_kernel, dim3((unsigned)grid), dim3(256), 2 * 4 * 8192, s, (const __bf16*)q, (const __bf16*)qd, ldq, q_bs,
                       (const __bf16*)k, (const __bf16*)v, (const __bf16*)kd, (const __bf16*)vd, ldk, kv_bs, (__bf16*)out, (__bf16*)outd, ldo, o_bs, Lq,
                       Lkv, 1.0f / sqrtf(128.0f), heads, B);
    WJ_RET();
}
int launch_wan_gelu_jvp(const void* h, const void* hd, void* a, void* ad, int64_t n, hipStream_t s) {
    if (n <= 0 || (n % 4) || (n / 4 + 255) / 256 > INT32_MAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(wan_gelu_jvp_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, (const __bf16*)h, (const __bf16*)hd, (__bf16*)a,
                       (__bf16*)ad, n / 4);
    WJ_RET();
}
int launch_wan_dup2(const float* tembd, float* modd, int rows, int D, hipStream_t s) {
    if (rows <= 0 || D <= 0) return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)rows * 2 * D;
    hipLaunchKernelGGL(wan_dup2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tembd, modd, rows, D);
    WJ_RET();
}
int launch_wan_final_jvp(int D, const void* x, const void* xd, const float* mod, const float* modd, const float* w, const float* bias, float* out,
                         float* outd, int ntok, int Fr, int gh, int gw, int C, float eps, hipStream_t s) {
    if (ntok <= 0 || Fr <= 0 || gh <= 0 || gw <= 0 || C <= 0) return (int)hipErrorInvalidValue;
    dim3 g((ntok + 3) / 4), b(256);
#define GO(NP)                                                                                                                                   \
    hipLaunchKernelGGL(wan_final_jvp_kernel<NP>, g, b, 0, s, (const __bf16*)x, (const __bf16*)xd, mod, modd, w, bias, out, outd, ntok, Fr, gh, gw, C, \
                       eps)
    WJ_SWITCH(D, GO)
#undef GO
    WJ_RET();
}
