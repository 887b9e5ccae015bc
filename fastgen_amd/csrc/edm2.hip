// EDM2 U-Net (reference fastgen/networks/EDM2/network.py) forward kernels besides the shared ADM convolution / attention: see edm2.h.
#include "edm2.h"
#include "common.h"

#include <math.h>

namespace {

#define RET_LAST() return (int)hipGetLastError()

// One workgroup per output row: the row's norm in fp32 (fixed-order tree: deterministic), then the scaled, padded copy.
__global__ __launch_bounds__(256) void edm2_prep_weight_kernel(const float* __restrict__ w, float* __restrict__ out, int cin, int cin_pad,
                                                               int taps, const float* __restrict__ gain, float extra0, float extra1,
                                                               int c_split) {
    __shared__ float red[256];
    const int o = blockIdx.x;
    const int64_t fan = (int64_t)cin * taps;
    const float* row = w + (size_t)o * fan;
    float ss = 0.f;
    for (int64_t i = threadIdx.x; i < fan; i += 256) ss = fmaf(row[i], row[i], ss);
    red[threadIdx.x] = ss;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    const float rs = sqrtf((float)fan);
    const float g = gain ? gain[0] : 1.0f;
    const float sc = g / rs / (1e-4f + sqrtf(red[0]) / rs);
    const int64_t fan_p = (int64_t)cin_pad * taps;
    for (int64_t i = threadIdx.x; i < fan_p; i += 256) {
        const int ci = (int)(i / taps), tap = (int)(i % taps);
        out[(size_t)o * fan_p + i] = ci < cin ? row[(size_t)ci * taps + tap] * (sc * (ci < c_split ? extra0 : extra1)) : 0.f;
    }
}

// One wave per output pixel; lanes stride the channels.
__global__ __launch_bounds__(256) void edm2_pixel_norm_kernel(const float* x, float* out, int B, int H, int C, int down) {
    const int lane = threadIdx.x & 63;
    const int64_t pix = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= (int64_t)B * H * H) return;
    const int b = (int)(pix / ((int64_t)H * H)), rem = (int)(pix % ((int64_t)H * H)), y = rem / H, xx = rem % H;
    auto load = [&](int c) -> float {
        if (!down) return x[(size_t)pix * C + c];
        const int R = 2 * H;
        const float* p = x + (((size_t)b * R + 2 * y) * R + 2 * xx) * C + c;
        const size_t rs = (size_t)R * C;
        return 0.25f * ((p[0] + p[C]) + (p[rs] + p[rs + C]));
    };
    float ss = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = load(c);
        ss = fmaf(v, v, ss);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    const float inv = 1.0f / (1e-4f + sqrtf(ss) / sqrtf((float)C));
    for (int c = lane; c < C; c += 64) out[(size_t)pix * C + c] = load(c) * inv;
}

__global__ void edm2_fourier_kernel(const float* __restrict__ c_noise, const float* __restrict__ freqs, const float* __restrict__ phases,
                                    float* __restrict__ out, int B, int N) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * N) return;
    const int b = idx / N, j = idx % N;
    const float y = c_noise[b] * freqs[j];
    out[idx] = cosf(y + phases[j]) * 1.41421356237309515f;  // np.sqrt(2) as fp32
}

__global__ void edm2_emb_finish_kernel(const float* __restrict__ e, const float* __restrict__ lab, float* __restrict__ out, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = silu_f<false>(e[i] + (lab ? lab[i] : 0.f)) / 0.596f;
}

__global__ void edm2_mod_rows_kernel(const float* __restrict__ c, float2* __restrict__ ab, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    ab[i] = make_float2(c[i] + 1.0f, 0.0f);
}

__global__ void edm2_stem_operand_kernel(const float* __restrict__ x, const float* __restrict__ c_in, float* __restrict__ out, int B, int C,
                                         int R, int Cp) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)B * R * R * Cp;
    if (idx >= total) return;
    const int c = (int)(idx % Cp);
    const int64_t pix = idx / Cp;
    const int b = (int)(pix / ((int64_t)R * R)), p = (int)(pix % ((int64_t)R * R));
    float v = 0.f;
    if (c < C) v = c_in[b] * x[((size_t)b * C + c) * R * R + p];
    else if (c == C) v = 1.0f;
    out[idx] = v;
}

__global__ void edm2_precond_out_kernel(const float* __restrict__ F, const float* __restrict__ x, const float* __restrict__ c_skip,
                                        const float* __restrict__ c_out, float* __restrict__ out, int B, int C, int R) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)B * C * R * R;
    if (idx >= total) return;
    const int p = (int)(idx % ((int64_t)R * R));
    const int c = (int)((idx / ((int64_t)R * R)) % C);
    const int b = (int)(idx / ((int64_t)C * R * R));
    out[idx] = c_skip[b] * x[idx] + c_out[b] * F[((size_t)b * R * R + p) * C + c];
}

unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

int edm2_launch_prep_weight(const float* w, float* out, int cout, int cin, int cin_pad, int taps, const float* gain, float extra0,
                            float extra1, int c_split, hipStream_t s) {
    if (cout <= 0 || cin <= 0 || cin_pad < cin || taps <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(edm2_prep_weight_kernel, dim3(cout), dim3(256), 0, s, w, out, cin, cin_pad, taps, gain, extra0, extra1, c_split);
    RET_LAST();
}

int edm2_launch_pixel_norm(const float* x, float* out, int B, int H, int C, int down, hipStream_t s) {
    if (B <= 0 || H <= 0 || C <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(edm2_pixel_norm_kernel, dim3(blocks_for((int64_t)B * H * H, 4)), dim3(256), 0, s, x, out, B, H, C, down);
    RET_LAST();
}

int edm2_launch_fourier(const float* c_noise, const float* freqs, const float* phases, float* out, int B, int N, hipStream_t s) {
    hipLaunchKernelGGL(edm2_fourier_kernel, dim3(blocks_for((int64_t)B * N, 256)), dim3(256), 0, s, c_noise, freqs, phases, out, B, N);
    RET_LAST();
}

int edm2_launch_emb_finish(const float* e, const float* lab, float* out, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(edm2_emb_finish_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, e, lab, out, n);
    RET_LAST();
}

int edm2_launch_mod_rows(const float* c, float2* ab, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(edm2_mod_rows_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, c, ab, n);
    RET_LAST();
}

int edm2_launch_stem_operand(const float* x_t, const float* c_in, float* out, int B, int C, int R, int Cp, hipStream_t s) {
    if (Cp < C + 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(edm2_stem_operand_kernel, dim3(blocks_for((int64_t)B * R * R * Cp, 256)), dim3(256), 0, s, x_t, c_in, out, B, C, R, Cp);
    RET_LAST();
}

int edm2_launch_precond_out(const float* F, const float* x_t, const float* c_skip, const float* c_out, float* out, int B, int C, int R,
                            hipStream_t s) {
    hipLaunchKernelGGL(edm2_precond_out_kernel, dim3(blocks_for((int64_t)B * C * R * R, 256)), dim3(256), 0, s, F, x_t, c_skip, c_out, out, B,
                       C, R);
    RET_LAST();
}
