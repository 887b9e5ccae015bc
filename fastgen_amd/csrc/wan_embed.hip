// The patch embedding of every Wan network: Conv3d(kernel = stride = (1,2,2)) + bias over a [B][Ct][Fr][H][W] fp32 input, tokens
// ordered (frame, row, column), bf16 out.  One fp32 fmaf chain per output over k = 0 .. 4 Ct - 1 (k = 4 c + 2 py + px, the weight's
// own order), started at the bias and rounded to bf16 once.  Every kernel here keeps that chain in that order, so they are
// bit-identical to each other; the tests assert it and pin the per-output kernel to fp64.
// Two things vary independently:
//   where input k of a token comes from   WanEmbedSrc (misc.h) through wan_embed_plane(), the only place that knows the three conventions
//   how the product is scheduled           three kernel templates; wan_embed_plan() picks one from (mode, Ct) alone
//   wan_embed_kernel<MODE>            one output element per thread, any Ct: the tests' reference (path 1)
//   wan_embed_rows_kernel<K, NOUT, MODE>   32 tokens' inputs in LDS as [token][k], NOUT adjacent outputs' whole weight rows in registers
//   wan_embed_phased_kernel<C>        32 tokens in LDS as [input quad][token], 2 x 32 running sums in registers, the two weight rows
//                                     taken in phases of 48 inputs (a 192- or 384-float row does not fit beside the sums)
// Token tok of sample b goes to row b * out_rows + (tok - b * per) of out, per = Fr gh gw <= out_rows: a caller may leave rows behind a
// sample's tokens (VACE's zero padding, VaceWan/network.py:81-88); those rows are never touched.
#include "common.h"
#include "misc.h"

namespace {

constexpr int TOK = 32;  // tokens per workgroup of the two tiled kernels

// The H x W plane of virtual channel c of frame f of sample b; nullptr (concat only): a mask channel.  C is the view's latent channel
// count and mode its mode; they are passed apart from the view so that a kernel instantiated for one value hands in its constant.
//   plain    x [B][C][Fr][H][W]
//   frame 0  the same with frame 0 read from alt [B][C][1][H][W]: the replaced latents of `_replace_first_frame`
//            (WanI2V/network.py:254-277) are never materialised
//   concat   [x (C) | mask (4) | alt (C)] with alt [B][C][Fr][H][W]: the mask is never materialised either - the reshuffle of
//            WanI2V/network.py:310-327 leaves ones on latent frame 0 and zeros elsewhere, on all four channels
// (One selected address: a load per branch keeps the callers' loads from being batched - 2.8 x on the per-output kernel.)
__device__ __forceinline__ const float* wan_embed_plane(const WanEmbedSrc& s, int mode, int C, int b, int c, int f) {
    const size_t hw = (size_t)s.H * s.W;
    if (mode == WAN_EMBED_CONCAT && c >= C && c < C + 4) return nullptr;
    const float* plane = s.x + (((size_t)b * C + c) * s.Fr + f) * hw;
    if (mode == WAN_EMBED_FRAME0 && f == 0) plane = s.alt + ((size_t)b * C + c) * hw;
    if (mode == WAN_EMBED_CONCAT && c >= C) plane = s.alt + (((size_t)b * C + (c - C - 4)) * s.Fr + f) * hw;
    return plane;
}
__device__ __forceinline__ float wan_embed_mask(int f) { return f == 0 ? 1.0f : 0.0f; }
// virtual channel c of frame f at pixel `pos` (= y W + x)
__device__ __forceinline__ float wan_embed_in(const WanEmbedSrc& s, int mode, int C, int b, int c, int f, size_t pos) {
    const float* plane = wan_embed_plane(s, mode, C, b, c, f);
    return mode == WAN_EMBED_CONCAT && !plane ? wan_embed_mask(f) : plane[pos];
}

struct WanEmbedTok {
    int b, f;
    size_t pos;  // of the token's top left pixel
};
__device__ __forceinline__ WanEmbedTok wan_embed_tok(const WanEmbedSrc& s, int64_t tok) {
    const int gw = s.W / 2, fs = (s.H / 2) * gw;
    const int hw = (int)(tok % fs), f = (int)((tok / fs) % s.Fr), b = (int)(tok / ((int64_t)fs * s.Fr));
    const int gy = hw / gw, gx = hw - gy * gw;
    return {b, f, (size_t)(2 * gy) * s.W + 2 * gx};
}

// The output rows of a tile's tokens, for the barrier behind the staging loop.  A table, not "the tile's first row and one sample
// boundary": a sample may have fewer than 32 tokens, and a division per token inside the product loops costs the rows kernel a third
// of its occupancy.  (A tail tile repeats the last token; its results are not stored.)
__device__ __forceinline__ void wan_embed_tile_rows(int64_t (&orow)[TOK], int64_t tok0, int64_t ntok, int64_t per, int64_t out_rows) {
    if (threadIdx.x < TOK) {
        const int64_t tok = tok0 + threadIdx.x < ntok ? tok0 + threadIdx.x : ntok - 1, b = tok / per;
        orow[threadIdx.x] = b * out_rows + (tok - b * per);
    }
}

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_;

template <int MODE>
__global__ __launch_bounds__(256) void wan_embed_kernel(WanEmbedSrc s, const float* __restrict__ w, const float* __restrict__ bias,
                                                        __bf16* __restrict__ out, int B, int D, int64_t out_rows) {
    const int Ct = MODE == WAN_EMBED_CONCAT ? 2 * s.C + 4 : s.C, W = s.W;
    const int64_t per = (int64_t)s.Fr * (s.H / 2) * (W / 2), total = B * per * D;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int d = (int)(i % D);
        const int64_t tok = i / D;
        const WanEmbedTok t = wan_embed_tok(s, tok);
        float a = bias[d];
        const float* wr = w + (size_t)d * Ct * 4;
        for (int c = 0; c < Ct; ++c) {
            const float* xp = wan_embed_plane(s, MODE, s.C, t.b, c, t.f);
            float x0, x1, x2, x3;
            if (MODE == WAN_EMBED_CONCAT && !xp) x0 = x1 = x2 = x3 = wan_embed_mask(t.f);
            else xp += t.pos, x0 = xp[0], x1 = xp[1], x2 = xp[W], x3 = xp[W + 1];
            a = fmaf(wr[c * 4 + 0], x0, a);
            a = fmaf(wr[c * 4 + 1], x1, a);
            a = fmaf(wr[c * 4 + 2], x2, a);
            a = fmaf(wr[c * 4 + 3], x3, a);
        }
        out[(size_t)(t.b * out_rows + (tok - t.b * per)) * D + d] = (__bf16)a;
    }
}

// K = 4 Ct inputs per token.  A workgroup stages 32 tokens' inputs in LDS and every thread keeps the weight rows of NOUT adjacent
// outputs in registers while it walks the 32 tokens (broadcast LDS reads): each weight row is fetched once per 32 tokens instead of
// once per token with scattered 4-byte loads.  <64, 2>: every 16-channel Wan 2.1 network (8 KiB); <144, 1>: Wan 2.1 I2V's virtual
// concat (18 KiB, one 144-float row is what the registers hold).  D % NOUT == 0.
template <int K, int NOUT, int MODE>
__global__ __launch_bounds__(256) void wan_embed_rows_kernel(WanEmbedSrc s, const float* __restrict__ w, const float* __restrict__ bias,
                                                             __bf16* __restrict__ out, int B, int D, int64_t out_rows) {
    static_assert(NOUT == 1 || NOUT == 2, "one output or a bf16 pair per store");
    constexpr int C = MODE == WAN_EMBED_CONCAT ? (K / 4 - 4) / 2 : K / 4;
    __shared__ __attribute__((aligned(16))) float xs[TOK][K];
    __shared__ int64_t orow[TOK];
    const int64_t per = (int64_t)s.Fr * (s.H / 2) * (s.W / 2), ntok = B * per, tok0 = (int64_t)blockIdx.x * TOK;
    const int tid = threadIdx.x;
#pragma unroll 8
    for (int i = 0; i < TOK * K / 256; ++i) {
        const int idx = tid + 256 * i, tl = idx / K, k = idx - tl * K, c = k >> 2, py = (k >> 1) & 1, px = k & 1;
        const WanEmbedTok t = wan_embed_tok(s, tok0 + tl < ntok ? tok0 + tl : ntok - 1);
        xs[tl][k] = wan_embed_in(s, MODE, C, t.b, c, t.f, t.pos + (size_t)py * s.W + px);
    }
    wan_embed_tile_rows(orow, tok0, ntok, per, out_rows);
    __syncthreads();
    for (int d = NOUT * tid; d < D; d += NOUT * 256) {
        f32x4 wr[NOUT][K / 4];
        float b0[NOUT];
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
#pragma unroll
            for (int q = 0; q < K / 4; ++q) wr[o][q] = *reinterpret_cast<const f32x4*>(w + (size_t)(d + o) * K + 4 * q);
            b0[o] = bias[d + o];
        }
        for (int t = 0; t < TOK && tok0 + t < ntok; ++t) {
            float a[NOUT];
#pragma unroll
            for (int o = 0; o < NOUT; ++o) a[o] = b0[o];
#pragma unroll
            for (int q = 0; q < K / 4; ++q) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(&xs[t][4 * q]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int o = 0; o < NOUT; ++o) a[o] = fmaf(wr[o][q][e], xv[e], a[o]);
            }
            __bf16* dst = out + (size_t)orow[t] * D + d;
            if (NOUT == 2) *reinterpret_cast<bf16x2_*>(dst) = bf16x2_{(__bf16)a[0], (__bf16)a[NOUT - 1]};
            else *dst = (__bf16)a[0];
        }
    }
}

// C = Ct real channels, K = 4 C inputs per token (48: Wan2.2 TI2V-5B, 24 KiB; 96: the VACE control video, 48 KiB), the view plain or
// frame 0 (read at run time).  A workgroup stages 32 tokens' inputs in LDS as [input quad][token], so that a wave's staging loads
// walk image rows and the product loop reads one quad per token as a broadcast; a thread owns two adjacent outputs and keeps their
// 32 + 32 running sums in registers while it takes the two weight rows in K / 48 phases of 48 inputs (96 weight registers).  D % 2 == 0.
template <int C>
__global__ __launch_bounds__(256) void wan_embed_phased_kernel(WanEmbedSrc s, const float* __restrict__ w, const float* __restrict__ bias,
                                                               __bf16* __restrict__ out, int B, int D, int64_t out_rows) {
    constexpr int K = 4 * C, QP = 12, NPH = K / (4 * QP);
    __shared__ f32x4 xs[K / 4][TOK];
    __shared__ int64_t orow[TOK];
    const int64_t per = (int64_t)s.Fr * (s.H / 2) * (s.W / 2), ntok = B * per, tok0 = (int64_t)blockIdx.x * TOK;
    const int tid = threadIdx.x, mode = s.mode == WAN_EMBED_FRAME0 ? WAN_EMBED_FRAME0 : WAN_EMBED_PLAIN;
    float* xsf = reinterpret_cast<float*>(&xs[0][0]);
#pragma unroll 4
    for (int i = 0; i < TOK * K / 256; ++i) {
        const int idx = tid + 256 * i, px = idx & 1, tl = (idx >> 1) & (TOK - 1), cp = idx >> 6, c = cp >> 1, py = cp & 1;
        const WanEmbedTok t = wan_embed_tok(s, tok0 + tl < ntok ? tok0 + tl : ntok - 1);
        xsf[((size_t)c * TOK + tl) * 4 + 2 * py + px] = wan_embed_in(s, mode, C, t.b, c, t.f, t.pos + (size_t)py * s.W + px);
    }
    wan_embed_tile_rows(orow, tok0, ntok, per, out_rows);
    __syncthreads();
    for (int d = 2 * tid; d < D; d += 512) {
        float a0[TOK], a1[TOK];
        const float b0 = bias[d], b1 = bias[d + 1];
#pragma unroll
        for (int t = 0; t < TOK; ++t) a0[t] = b0, a1[t] = b1;
#pragma unroll 1
        for (int ph = 0; ph < NPH; ++ph) {
            f32x4 w0[QP], w1[QP];
#pragma unroll
            for (int q = 0; q < QP; ++q) {
                w0[q] = *reinterpret_cast<const f32x4*>(w + (size_t)d * K + 4 * (ph * QP + q));
                w1[q] = *reinterpret_cast<const f32x4*>(w + (size_t)(d + 1) * K + 4 * (ph * QP + q));
            }
#pragma unroll
            for (int t = 0; t < TOK; ++t)
#pragma unroll
                for (int q = 0; q < QP; ++q) {
                    const f32x4 xv = xs[ph * QP + q][t];
#pragma unroll
                    for (int e = 0; e < 4; ++e) a0[t] = fmaf(w0[q][e], xv[e], a0[t]), a1[t] = fmaf(w1[q][e], xv[e], a1[t]);
                }
        }
        // (the table is read behind the product loop: hoisted above it, its 64 registers ride through the loop - 238 VGPRs and 2 waves
        // per SIMD instead of 89 and 5 at C = 48, 30 % of the kernel's time)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int t = 0; t < TOK; ++t)
            if (tok0 + t < ntok) *reinterpret_cast<bf16x2_*>(out + (size_t)orow[t] * D + d) = bf16x2_{(__bf16)a0[t], (__bf16)a1[t]};
    }
}

// The one rule: the fast instances that exist, by (mode, Ct) alone; everything else runs per output.
enum WanEmbedPlan { PER_OUTPUT, ROWS_64_2, ROWS_144_1, PHASED_48, PHASED_96 };
WanEmbedPlan wan_embed_plan(int mode, int Ct) {
    if (mode == WAN_EMBED_PLAIN && Ct == 16) return ROWS_64_2;
    if (mode == WAN_EMBED_CONCAT && Ct == 36) return ROWS_144_1;
    if (mode != WAN_EMBED_CONCAT && Ct == 48) return PHASED_48;
    if (mode == WAN_EMBED_PLAIN && Ct == 96) return PHASED_96;
    return PER_OUTPUT;
}

}  // namespace

int launch_wan_embed(const WanEmbedSrc& src, const float* w, const float* bias, void* out, int B, int D, int64_t out_rows, int path, hipStream_t s) {
    if (!src.x || src.mode < WAN_EMBED_PLAIN || src.mode > WAN_EMBED_CONCAT || (src.mode != WAN_EMBED_PLAIN && !src.alt) || !w || !bias || !out ||
        path < 0 || path > 2 || B <= 0 || src.C <= 0 || src.Fr <= 0 || src.H <= 0 || src.W <= 0 || (src.H & 1) || (src.W & 1) || D <= 0)
        return (int)hipErrorInvalidValue;
    const int64_t per = (int64_t)src.Fr * (src.H / 2) * (src.W / 2), ntok = B * per;
    if (out_rows < per) return (int)hipErrorInvalidValue;
    const WanEmbedPlan plan = path == 1 ? PER_OUTPUT : wan_embed_plan(src.mode, src.mode == WAN_EMBED_CONCAT ? 2 * src.C + 4 : src.C);
    if (path == 2 && plan != PHASED_48 && plan != PHASED_96) return (int)hipErrorInvalidValue;
    if (plan != PER_OUTPUT && plan != ROWS_144_1 && (D & 1)) return (int)hipErrorInvalidValue;  // (these store bf16 pairs)
    const int64_t blocks = (ntok * D + 255) / 256;
    const dim3 grid((unsigned)(plan == PER_OUTPUT ? (blocks > 262144 ? 262144 : blocks) : (ntok + TOK - 1) / TOK));
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, src, w, bias, (__bf16*)out, B, D, out_rows); };
    switch (plan) {
    case ROWS_64_2: launch(wan_embed_rows_kernel<64, 2, WAN_EMBED_PLAIN>); break;
    case ROWS_144_1: launch(wan_embed_rows_kernel<144, 1, WAN_EMBED_CONCAT>); break;
    case PHASED_48: launch(wan_embed_phased_kernel<48>); break;
    case PHASED_96: launch(wan_embed_phased_kernel<96>); break;
    case PER_OUTPUT:
        if (src.mode == WAN_EMBED_PLAIN) launch(wan_embed_kernel<WAN_EMBED_PLAIN>);
        else if (src.mode == WAN_EMBED_FRAME0) launch(wan_embed_kernel<WAN_EMBED_FRAME0>);
        else launch(wan_embed_kernel<WAN_EMBED_CONCAT>);
        break;
    }
    return (int)hipGetLastError();
}
