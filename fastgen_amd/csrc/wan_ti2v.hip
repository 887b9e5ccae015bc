// Wan2.2 TI2V-5B (reference fastgen/networks/WanI2V/network.py, concat_mask = False, expand_timesteps = True; Wan/network.py with 48
// latent channels): the output head at 48 channels, where 4 C = 192 outputs per token make the wave-per-token head of wan.hip re-read
// its whole weight once per token, and the first-frame mask of the time embedder.  (The patch embedding is wan_embed.hip.)
//   wan_ti2v_final48_kernel        LayerNorm -> modulate -> proj_out (D -> 192) -> un-patchify on 32-token tiles: an fp32 tile
//                                   product with the normalised tokens and the weight staged through LDS in chunks of 32 inputs
//   wan_ti2v_zero_frame0_kernel     the embedder rows of latent frame 0 set to zero (`_compute_timestep_inputs` under the
//                                   first-frame mask, WanI2V/network.py:334-340)
// The optional second source `ff0` [B][C][1][H][W] is the first-frame condition: the head writes it into frame 0 of its result (the
// replaced latents of `_replace_first_frame`, :254-277, are never materialised; the embedding reads frame 0's tokens from it).
#include "common.h"
#include "misc.h"

namespace {

__device__ __forceinline__ float wsum_ti2v(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// LayerNorm(eps, no affine) -> (1 + scale) y + shift with mod[tok / (gh gw)] = {shift, scale} [2][D] -> proj_out -> un-patchify for 48
// channels: out [B][48][F][H][W] fp32, feature o = (py 2 + px) 48 + c.  A workgroup owns 32 tokens: two-pass fp32 statistics (one
// wave per token, eight tokens per wave), then the [32 tokens] x [192 outputs] product over D in chunks of 32 inputs - the modulated
// tokens (fp32) and the weight chunk go through LDS (rows padded to 36 floats: 16 consecutive rows cover all banks once), the next
// chunk's global loads are in flight while the current one is multiplied.  A thread holds 4 tokens x 6 outputs; every sum runs k
// upwards from zero, the bias is added last (as wan_final_kernel adds it).
__global__ __launch_bounds__(256) void wan_ti2v_final48_kernel(const __bf16* __restrict__ x, const float* __restrict__ mod, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const float* __restrict__ ff0,
                                                               float* __restrict__ out, int ntok, int Fr, int gh, int gw, int D, float eps) {
    constexpr int C = 48, NO = 4 * C, TOK = 32, KC = 32, LD = KC + 4, TI = 4, JO = NO / 32, WL = NO * (KC / 4) / 256;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_;
    __shared__ __attribute__((aligned(16))) float ys[TOK][LD];
    __shared__ __attribute__((aligned(16))) float ws[NO][LD];
    __shared__ float s_mean[TOK], s_rstd[TOK];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tok0 = blockIdx.x * TOK, fs = gh * gw;
    for (int i = 0; i < TOK / 4; ++i) {
        const int tl = wv * (TOK / 4) + i, tok = tok0 + tl < ntok ? tok0 + tl : ntok - 1;
        const __bf16* row = x + (size_t)tok * D;
        float s = 0.f;
        for (int c = 2 * lane; c < D; c += 128) {
            const bf16x2_ q = *reinterpret_cast<const bf16x2_*>(row + c);
            s += (float)q[0] + (float)q[1];
        }
        const float mean = wsum_ti2v(s) * (1.0f / D);
        float ss = 0.f;
        for (int c = 2 * lane; c < D; c += 128) {
            const bf16x2_ q = *reinterpret_cast<const bf16x2_*>(row + c);
            const float u0 = (float)q[0] - mean, u1 = (float)q[1] - mean;
            ss = fmaf(u0, u0, ss);
            ss = fmaf(u1, u1, ss);
        }
        const float rstd = 1.0f / sqrtf(wsum_ti2v(ss) * (1.0f / D) + eps);
        if (lane == 0) s_mean[tl] = mean, s_rstd[tl] = rstd;
    }
    __syncthreads();
    // staging roles: one token quad of the chunk, and WL weight quads
    const int y_tl = tid >> 3, y_k = (tid & 7) * 4;
    const int y_tok = tok0 + y_tl < ntok ? tok0 + y_tl : ntok - 1;
    const float y_mean = s_mean[y_tl], y_rstd = s_rstd[y_tl];
    const __bf16* y_row = x + (size_t)y_tok * D + y_k;
    const float* y_mod = mod + (size_t)(y_tok / fs) * 2 * D + y_k;
    bf16x4 rx;
    f32x4 rsh, rsc, rw[WL];
    auto fetch = [&](int k0) {
        rx = *reinterpret_cast<const bf16x4*>(y_row + k0);
        rsh = *reinterpret_cast<const f32x4*>(y_mod + k0);
        rsc = *reinterpret_cast<const f32x4*>(y_mod + D + k0);
#pragma unroll
        for (int i = 0; i < WL; ++i) {
            const int idx = tid + 256 * i;
            rw[i] = *reinterpret_cast<const f32x4*>(w + (size_t)(idx >> 3) * D + k0 + (idx & 7) * 4);
        }
    };
    const int to = tid & 31, tt = tid >> 5;
    float acc[TI][JO];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < JO; ++j) acc[i][j] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < D; k0 += KC) {
        f32x4 yv;
#pragma unroll
        for (int e = 0; e < 4; ++e) yv[e] = fmaf(((float)rx[e] - y_mean) * y_rstd, 1.0f + rsc[e], rsh[e]);
        *reinterpret_cast<f32x4*>(&ys[y_tl][y_k]) = yv;
#pragma unroll
        for (int i = 0; i < WL; ++i) {
            const int idx = tid + 256 * i;
            *reinterpret_cast<f32x4*>(&ws[idx >> 3][(idx & 7) * 4]) = rw[i];
        }
        __syncthreads();
        if (k0 + KC < D) fetch(k0 + KC);
#pragma unroll
        for (int kk = 0; kk < KC; kk += 4) {
            f32x4 a[TI], bq[JO];
#pragma unroll
            for (int i = 0; i < TI; ++i) a[i] = *reinterpret_cast<const f32x4*>(&ys[tt * TI + i][kk]);
#pragma unroll
            for (int j = 0; j < JO; ++j) bq[j] = *reinterpret_cast<const f32x4*>(&ws[to + 32 * j][kk]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TI; ++i)
#pragma unroll
                    for (int j = 0; j < JO; ++j) acc[i][j] = fmaf(a[i][e], bq[j][e], acc[i][j]);
        }
        __syncthreads();
    }
    const int H = 2 * gh, W = 2 * gw;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        const int tok = tok0 + tt * TI + i;
        if (tok >= ntok) continue;
        const int bf = tok / fs, hw = tok - bf * fs, b = bf / Fr, f = bf - b * Fr, gy = hw / gw, gx = hw - gy * gw;
#pragma unroll
        for (int j = 0; j < JO; ++j) {
            const int o = to + 32 * j, c = o % C, pq = o / C, py = pq >> 1, px = pq & 1;
            const size_t pos = (size_t)(2 * gy + py) * W + 2 * gx + px;
            const float v = (ff0 && f == 0) ? ff0[((size_t)b * C + c) * H * W + pos] : acc[i][j] + bias[o];
            out[(((size_t)b * C + c) * Fr + f) * H * W + pos] = v;
        }
    }
}

__global__ void wan_ti2v_zero_frame0_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int Fr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (i % Fr) == 0 ? 0.0f : src[i];
}

}  // namespace

int launch_wan_ti2v_final(int D, const void* x, const float* mod, const float* w, const float* bias, const float* ff0, float* out, int ntok, int Fr,
                          int gh, int gw, int C, float eps, int path, hipStream_t s) {
    if (path < 0 || path > 2 || ntok <= 0 || Fr <= 0 || gh <= 0 || gw <= 0 || C <= 0 || D <= 0 || (ntok % (Fr * gh * gw)))
        return (int)hipErrorInvalidValue;
    const bool tiled_ok = C == 48 && (D % 32) == 0;
    if (path == 2 && !tiled_ok) return (int)hipErrorInvalidValue;
    if (tiled_ok && path != 1) {
        hipLaunchKernelGGL(wan_ti2v_final48_kernel, dim3((unsigned)((ntok + 31) / 32)), dim3(256), 0, s, (const __bf16*)x, mod, w, bias, ff0, out,
                           ntok, Fr, gh, gw, D, eps);
        return (int)hipGetLastError();
    }
    const int rc = launch_wan_final(D, x, mod, w, bias, out, ntok, Fr, gh, gw, C, eps, s);
    if (rc || !ff0) return rc;
    // frame 0 of every (sample, channel) plane from the second source, behind the head on the same stream
    const int64_t hw = (int64_t)4 * gh * gw;
    return launch_copy_rows(ff0, hw, out, (int64_t)Fr * hw, hw, (int64_t)(ntok / (Fr * gh * gw)) * C, s);
}

int launch_wan_ti2v_zero_frame0(const float* src, float* dst, int n, int Fr, hipStream_t s) {
    hipLaunchKernelGGL(wan_ti2v_zero_frame0_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, n, Fr);
    return (int)hipGetLastError();
}
