// VACE (reference fastgen/networks/VaceWan/network.py; diffusers' WanVACETransformer3DModel): the two ends of the control branch.  Its
// hot path is the block kernels of wan.hip / gemm.hip / attn.hip on a second token stream (engine_wan.inc: one block body serves both
// streams); what is new is where that stream begins.
//   wan_vace_patch_embed96_kernel   vace_patch_embedding: Conv3d(96 -> D, kernel = stride = (1,2,2)) + bias on 32-token tiles staged in
//                                   LDS, K = 384 inputs per token; every weight row is fetched once per tile, where the per-output
//                                   kernel of wan.hip re-reads a 384-float row per output element.  The fmaf chain of
//                                   wan_patch_embed_kernel in its order: bit-identical to it.
//   wan_vace_seed_kernel            c = ctx_in + x0, the control stream's first state (proj_in is applied once per context by
//                                   fg_wan_set_vace_context), one pass with 16-byte accesses
//   wan_vace_scale_rows_kernel      the hint scales as [n][D] fp32 gate rows of the injection GEMM
// The embedding writes sample b's tokens to rows [b * out_rows, b * out_rows + Fc gh gw) of its output: the context may have fewer
// frames than the video, and the rows behind them (zero padding, written by the caller) are never touched - frames beyond Fc are not read.
#include "common.h"
#include "misc.h"

namespace {

// x [B][96][Fc][H][W] fp32 -> tokens bf16, D per row.  The plan of wan_ti2v_patch_embed48_kernel at twice the channels: a workgroup
// stages 32 tokens' inputs in LDS (96 quads x 32 tokens x 16 B = 48 KiB, as [input quad][token]: a wave's staging loads walk image rows
// and the product loop reads one quad per token as a broadcast); a thread owns two adjacent outputs and keeps their 32 + 32 running
// sums in registers while it takes the two weight rows in eight phases of 48 inputs (96 weight registers: a 384-float row does not fit
// beside the sums).  Per output the sum runs k = 0 .. 383 upwards from the bias, as wan_patch_embed_kernel's.
__global__ __launch_bounds__(256) void wan_vace_patch_embed96_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                     const float* __restrict__ bias, __bf16* __restrict__ out, int B, int Fc, int H,
                                                                     int W, int D, int64_t out_rows) {
    constexpr int C = 96, K = 4 * C, TOK = 32, QP = 12, NPH = K / (4 * QP);
    __shared__ f32x4 xs[K / 4][TOK];
    const int gh = H / 2, gw = W / 2, fs = gh * gw;
    const int64_t per = (int64_t)Fc * fs, ntok = (int64_t)B * per, tok0 = (int64_t)blockIdx.x * TOK;
    const int tid = threadIdx.x;
    float* xsf = reinterpret_cast<float*>(&xs[0][0]);
#pragma unroll 4
    for (int i = 0; i < TOK * K / 256; ++i) {
        const int idx = tid + 256 * i, px = idx & 1, tl = (idx >> 1) & (TOK - 1), cp = idx >> 6, c = cp >> 1, py = cp & 1;
        const int64_t tok = tok0 + tl < ntok ? tok0 + tl : ntok - 1;  // (a tail tile repeats the last token; its results are not stored)
        const int hw = (int)(tok % fs), f = (int)((tok / fs) % Fc), b = (int)(tok / per);
        const int gy = hw / gw, gx = hw - gy * gw;
        const size_t pos = (size_t)(2 * gy + py) * W + 2 * gx + px;
        xsf[((size_t)c * TOK + tl) * 4 + 2 * py + px] = x[(((size_t)b * C + c) * Fc + f) * H * W + pos];
    }
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
        typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_;
#pragma unroll
        for (int t = 0; t < TOK; ++t) {
            const int64_t tok = tok0 + t;
            if (tok < ntok) {
                const int64_t b = tok / per, row = b * out_rows + (tok - b * per);
                *reinterpret_cast<bf16x2_*>(out + (size_t)row * D + d) = bf16x2_{(__bf16)a0[t], (__bf16)a1[t]};
            }
        }
    }
}

// c = a + b over n8 groups of eight bf16 (fp32 sum, rounded once)
__global__ __launch_bounds__(256) void wan_vace_seed_kernel(const __bf16* __restrict__ a, const __bf16* __restrict__ b, __bf16* __restrict__ c,
                                                            int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const bf16x8 u = *reinterpret_cast<const bf16x8*>(a + 8 * i), v = *reinterpret_cast<const bf16x8*>(b + 8 * i);
        bf16x8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (__bf16)((float)u[e] + (float)v[e]);
        *reinterpret_cast<bf16x8*>(c + 8 * i) = r;
    }
}

__global__ void wan_vace_scale_rows_kernel(WanVaceScales sc, float* __restrict__ rows, int n, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * D) rows[i] = sc.v[i / D];
}

}  // namespace

int launch_wan_vace_patch_embed(const float* x, const float* w, const float* bias, void* out, int B, int C, int Fc, int H, int W, int D,
                                int64_t out_rows, int path, hipStream_t s) {
    if (path < 0 || path > 2 || B <= 0 || C <= 0 || Fc <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || D <= 0) return (int)hipErrorInvalidValue;
    const int64_t per = (int64_t)Fc * (H / 2) * (W / 2), ntok = (int64_t)B * per;
    if (out_rows < per) return (int)hipErrorInvalidValue;
    const bool tiled_ok = C == 96 && (D % 2) == 0;
    if (path == 2 && !tiled_ok) return (int)hipErrorInvalidValue;
    if (tiled_ok && path != 1) {
        hipLaunchKernelGGL(wan_vace_patch_embed96_kernel, dim3((unsigned)((ntok + 31) / 32)), dim3(256), 0, s, x, w, bias, (__bf16*)out, B, Fc, H, W, D,
                           out_rows);
        return (int)hipGetLastError();
    }
    if (out_rows == per) return launch_wan_patch_embed(x, w, bias, out, B, C, Fc, H, W, D, s);
    for (int b = 0; b < B; ++b)  // (the per-output kernel writes one contiguous token block: a launch per sample)
        if (int rc = launch_wan_patch_embed(x + (size_t)b * C * Fc * H * W, w, bias, (__bf16*)out + (size_t)b * out_rows * D, 1, C, Fc, H, W, D, s)) return rc;
    return (int)hipSuccess;
}

int launch_wan_vace_seed(const void* ctx_in, const void* x0, void* c, int64_t n, hipStream_t s) {
    if (n <= 0 || (n % 8)) return (int)hipErrorInvalidValue;
    const int64_t n8 = n / 8, blocks = (n8 + 255) / 256;
    hipLaunchKernelGGL(wan_vace_seed_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, (const __bf16*)ctx_in, (const __bf16*)x0,
                       (__bf16*)c, n8);
    return (int)hipGetLastError();
}

int launch_wan_vace_scale_rows(const WanVaceScales& sc, float* rows, int n, int D, hipStream_t s) {
    if (n <= 0 || n > 64 || D <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(wan_vace_scale_rows_kernel, dim3((unsigned)((n * D + 255) / 256)), dim3(256), 0, s, sc, rows, n, D);
    return (int)hipGetLastError();
}
