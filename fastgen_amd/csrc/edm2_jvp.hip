// Forward-mode derivative (jvp) of the EDM2 U-Net: the tangent kernels beside edm2.hip and the shared ADM convolution / attention.
// Every kernel reads the primal values the forward kernels produced and writes tangents only (the attention may also write the primal
// output); the forward path is untouched.  fp32 NHWC activations.  See edm2.h.
#include "edm2.h"
#include "common.h"

#include <math.h>

namespace {

constexpr int NTHR = 256;
constexpr int AKT = 32;  // keys per tile, as adm_attention_kernel

#define RET_LAST() return (int)hipGetLastError()

unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// d/dz silu(z) = s (1 + z (1 - s)), s = sigmoid(z)
__device__ __forceinline__ float dsilu_f(float z) {
    const float s = 1.0f / (1.0f + expf(-z));
    return s * fmaf(z, 1.0f - s, 1.0f);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Cosine attention jvp, head dim 64, a VALU kernel in the form of adm_attention_kernel<true>: workgroup = 64 queries of one
// (image, head), key tiles of 32 through LDS, thread (tq, tk) = (tid / 16, tid % 16).  Beside every primal tile (Q^, K^ / 8, V^, P)
// sits its tangent (Q^_d, K^_d / 8, V^_d, P s_d); per query the running m, l, o = sum p v^, u = sum p s_d and wz = sum p (s_d v^ +
// v^_d) share one rescale.  The primal arithmetic repeats adm_attention_kernel<true> operation for operation, so `out` is the
// forward's to the bit.  LDS 83.7 KB: one workgroup (four waves) per CU.

// Rows [0, n) of the raw tile x ([*][pitch]) and of its raw tangent xd: xd <- xd / nrm - x (x . xd) / (8 |x| nrm^2) (0 where
// |x| = 0), then x <- x / nrm, nrm = 1e-4 + |x| / 8.  Four threads per row; the primal part is adm.hip's mp_norm_rows.
__device__ __forceinline__ void mp_norm_rows_jvp(float* x, float* xd, int pitch, int n, int tid) {
    const int row = tid >> 2, part = tid & 3;
    float ss = 0.f, dot = 0.f;
    if (row < n) {
        const float* p = x + (size_t)row * pitch + part * 16;
        const float* pd = xd + (size_t)row * pitch + part * 16;
#pragma unroll
        for (int d = 0; d < 16; ++d) ss = fmaf(p[d], p[d], ss);
#pragma unroll
        for (int d = 0; d < 16; ++d) dot = fmaf(p[d], pd[d], dot);
    }
    ss += __shfl_xor(ss, 1);
    ss += __shfl_xor(ss, 2);
    dot += __shfl_xor(dot, 1);
    dot += __shfl_xor(dot, 2);
    __syncthreads();
    if (row < n) {
        const float nx = sqrtf(ss);
        const float inv = 1.0f / (1e-4f + nx * 0.125f);
        const float proj = nx > 0.f ? dot * 0.125f * inv * inv / nx : 0.f;
        float* p = x + (size_t)row * pitch + part * 16;
        float* pd = xd + (size_t)row * pitch + part * 16;
#pragma unroll
        for (int d = 0; d < 16; ++d) {
            pd[d] = fmaf(pd[d], inv, -p[d] * proj);
            p[d] *= inv;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(NTHR) void edm2_attention_mp_jvp_kernel(const float* __restrict__ qkv, const float* __restrict__ qkv_d,
                                                                     float* __restrict__ out, float* __restrict__ out_d, int T, int heads) {
    __shared__ float Qs[64][65], Qd[64][65];                                   // [q][d]
    __shared__ float Ks[AKT][65], Kd[AKT][65];                                 // [k][d], scaled by 1/8 after the normalisation
    __shared__ float Vs[AKT][64], Vd[AKT][64];                                 // [k][d]
    __shared__ __attribute__((aligned(16))) float Pt[AKT][68], Pd[AKT][68];    // [k][q]: p and p s_d
    const int tid = threadIdx.x, tq = tid >> 4, tk = tid & 15;
    const int q0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
    const int C = heads * 64, C3 = 3 * C;
    const size_t hoff = (size_t)b * T * C3 + h * 192;
    const float* base = qkv + hoff;
    const float* based = qkv_d + hoff;
    for (int e = tid; e < 64 * 64; e += NTHR) {
        const int q = e >> 6, d = e & 63;
        Qs[q][d] = base[(size_t)(q0 + q) * C3 + 3 * d];
        Qd[q][d] = based[(size_t)(q0 + q) * C3 + 3 * d];
    }
    __syncthreads();
    mp_norm_rows_jvp(&Qs[0][0], &Qd[0][0], 65, 64, tid);
    float m[4], l[4], u[4], o[4][4], wz[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m[i] = -INFINITY;
        l[i] = 0.f;
        u[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[i][j] = 0.f, wz[i][j] = 0.f;
    }
    for (int k0 = 0; k0 < T; k0 += AKT) {
        for (int e = tid; e < AKT * 64; e += NTHR) {
            const int k = e >> 6, d = e & 63;
            const size_t off = (size_t)(k0 + k) * C3 + 3 * d;
            Ks[k][d] = base[off + 1];
            Vs[k][d] = base[off + 2];
            Kd[k][d] = based[off + 1];
            Vd[k][d] = based[off + 2];
        }
        __syncthreads();
        // rows 0..31 of (Ks, Kd), then of (Vs, Vd): one call, so every wave meets the same barriers
        mp_norm_rows_jvp(tid < 128 ? &Ks[0][0] : &Vs[0][0], tid < 128 ? &Kd[0][0] : &Vd[0][0], tid < 128 ? 65 : 64, AKT, tid & 127);
        for (int e = tid; e < AKT * 64; e += NTHR) {
            Ks[e >> 6][e & 63] *= 0.125f;
            Kd[e >> 6][e & 63] *= 0.125f;
        }
        __syncthreads();
        float s[4][2], sd[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i][0] = s[i][1] = sd[i][0] = sd[i][1] = 0.f;
#pragma unroll 8
        for (int d = 0; d < 64; ++d) {
            float qv[4], qd[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) qv[i] = Qs[4 * tq + i][d], qd[i] = Qd[4 * tq + i][d];
            const float k0v = Ks[tk][d], k1v = Ks[tk + 16][d];
            const float k0d = Kd[tk][d], k1d = Kd[tk + 16][d];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[i][0] = fmaf(qv[i], k0v, s[i][0]);
                s[i][1] = fmaf(qv[i], k1v, s[i][1]);
                sd[i][0] = fmaf(qd[i], k0v, fmaf(qv[i], k0d, sd[i][0]));
                sd[i][1] = fmaf(qd[i], k1v, fmaf(qv[i], k1d, sd[i][1]));
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float mx = fmaxf(s[i][0], s[i][1]);
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
            const float mn = fmaxf(m[i], mx);
            const float alpha = expf(m[i] - mn);
            const float p0 = expf(s[i][0] - mn), p1 = expf(s[i][1] - mn);
            const float g0 = p0 * sd[i][0], g1 = p1 * sd[i][1];
            Pt[tk][4 * tq + i] = p0;
            Pt[tk + 16][4 * tq + i] = p1;
            Pd[tk][4 * tq + i] = g0;
            Pd[tk + 16][4 * tq + i] = g1;
            float rs = p0 + p1, ru = g0 + g1;
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                rs += __shfl_xor(rs, off);
                ru += __shfl_xor(ru, off);
            }
            l[i] = l[i] * alpha + rs;
            u[i] = u[i] * alpha + ru;
            m[i] = mn;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[i][j] *= alpha, wz[i][j] *= alpha;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < AKT; ++k) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(&Pt[k][4 * tq]);
            const f32x4 gv = *reinterpret_cast<const f32x4*>(&Pd[k][4 * tq]);
            float vv[4], vd[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) vv[j] = Vs[k][tk + 16 * j], vd[j] = Vd[k][tk + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    o[i][j] = fmaf(pv[i], vv[j], o[i][j]);
                    wz[i][j] = fmaf(gv[i], vv[j], fmaf(pv[i], vd[j], wz[i][j]));
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float inv = 1.0f / l[i];
        const float ul = u[i] * inv;
        const size_t row = ((size_t)b * T + q0 + 4 * tq + i) * C + h * 64;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ov = o[i][j] * inv;
            if (out) out[row + tk + 16 * j] = ov;
            out_d[row + tk + 16 * j] = fmaf(-ul, ov, wz[i][j] * inv);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Pixel norm jvp: one wave per output pixel, lanes stride the channels (edm2_pixel_norm_kernel's walk).
__global__ __launch_bounds__(256) void edm2_pixel_norm_jvp_kernel(const float* x, const float* xd, float* out_d, int B, int H, int C, int down) {
    const int lane = threadIdx.x & 63;
    const int64_t pix = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= (int64_t)B * H * H) return;
    const int b = (int)(pix / ((int64_t)H * H)), rem = (int)(pix % ((int64_t)H * H)), y = rem / H, xx = rem % H;
    auto load = [&](const float* src, int c) -> float {
        if (!down) return src[(size_t)pix * C + c];
        const int R = 2 * H;
        const float* p = src + (((size_t)b * R + 2 * y) * R + 2 * xx) * C + c;
        const size_t rs = (size_t)R * C;
        return 0.25f * ((p[0] + p[C]) + (p[rs] + p[rs + C]));
    };
    float ss = 0.f, dot = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = load(x, c);
        ss = fmaf(v, v, ss);
        dot = fmaf(v, load(xd, c), dot);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ss += __shfl_xor(ss, off);
        dot += __shfl_xor(dot, off);
    }
    const float rc = sqrtf((float)C), nx = sqrtf(ss);
    const float inv = 1.0f / (1e-4f + nx / rc);
    const float proj = nx > 0.f ? dot * inv * inv / (rc * nx) : 0.f;
    // every lane has read all it needs of its own channels before it writes them: in place (down == 0) is safe
    for (int c = lane; c < C; c += 64) out_d[(size_t)pix * C + c] = fmaf(load(xd, c), inv, -load(x, c) * proj);
}

// out[b][p][c] = silu'(a x + b0) (a x_d + a_d x) over the virtual concat [x1 (C1) | x2 (C2)], {a, b0} = ab[b * ab_stride + c],
// a_d = ad ? ad[b * ad_stride + c] : 0.  Four channels per thread.
__global__ __launch_bounds__(256) void edm2_silu_operand_jvp_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                                    const float* __restrict__ d1, const float* __restrict__ d2, int C1, int C2,
                                                                    const float2* __restrict__ ab, int ab_stride, const float* __restrict__ ad,
                                                                    int ad_stride, float* __restrict__ out, int64_t hw, int64_t total4) {
    const int C = C1 + C2, Q = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % Q) * 4;
        const int64_t pix = i / Q;
        const int b = (int)(pix / hw);
        const size_t src = c < C1 ? (size_t)pix * C1 + c : (size_t)pix * C2 + (c - C1);
        const f32x4 xv = *reinterpret_cast<const f32x4*>((c < C1 ? x1 : x2) + src);
        const f32x4 dv = *reinterpret_cast<const f32x4*>((c < C1 ? d1 : d2) + src);
        const float2* row = ab + (size_t)b * ab_stride + c;
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 k = row[j];
            const float a_d = ad ? ad[(size_t)b * ad_stride + c + j] : 0.f;
            r[j] = dsilu_f(fmaf(xv[j], k.x, k.y)) * fmaf(k.x, dv[j], a_d * xv[j]);
        }
        *reinterpret_cast<f32x4*>(out + (size_t)pix * C + c) = r;
    }
}

// MPFourier tangent: out[b][j] = -sqrt(2) sin(c_noise[b] freqs[j] + phases[j]) freqs[j] c_noise_d[b]
__global__ void edm2_fourier_jvp_kernel(const float* __restrict__ c_noise, const float* __restrict__ c_noise_d, const float* __restrict__ freqs,
                                        const float* __restrict__ phases, float* __restrict__ out, int B, int N) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * N) return;
    const int b = idx / N, j = idx % N;
    const float y = c_noise[b] * freqs[j];
    out[idx] = -1.41421356237309515f * sinf(y + phases[j]) * freqs[j] * c_noise_d[b];
}

// mp_silu tangent of the embedding: out = silu'(e + lab) / 0.596 * e_d (the label part has no tangent)
__global__ void edm2_emb_finish_jvp_kernel(const float* __restrict__ e, const float* __restrict__ lab, const float* __restrict__ e_d,
                                           float* __restrict__ out, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = dsilu_f(e[i] + (lab ? lab[i] : 0.f)) / 0.596f * e_d[i];
}

__global__ void edm2_stem_operand_jvp_kernel(const float* __restrict__ x, const float* __restrict__ vx, const float* __restrict__ c_in,
                                             const float* __restrict__ c_in_d, float* __restrict__ out, int B, int C, int R, int Cp) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)B * R * R * Cp;
    if (idx >= total) return;
    const int c = (int)(idx % Cp);
    const int64_t pix = idx / Cp;
    const int b = (int)(pix / ((int64_t)R * R)), p = (int)(pix % ((int64_t)R * R));
    float v = 0.f;  // the ones channel is constant: tangent 0
    if (c < C) {
        const size_t s = ((size_t)b * C + c) * R * R + p;
        v = fmaf(c_in[b], vx[s], c_in_d[b] * x[s]);
    }
    out[idx] = v;
}

// clamp tangent: y is the clamped primal output; |y| >= clip: the clamp is (taken as) active
__global__ void edm2_clamp_jvp_kernel(const float* __restrict__ y, float* __restrict__ y_d, float clip, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (fabsf(y[i]) >= clip) y_d[i] = 0.f;
}

__global__ void edm2_precond_out_jvp_kernel(const float* __restrict__ F, const float* __restrict__ F_d, const float* __restrict__ x,
                                            const float* __restrict__ vx, const float* __restrict__ c_skip, const float* __restrict__ c_skip_d,
                                            const float* __restrict__ c_out, const float* __restrict__ c_out_d, float* __restrict__ jvp, int B,
                                            int C, int R) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)B * C * R * R;
    if (idx >= total) return;
    const int p = (int)(idx % ((int64_t)R * R));
    const int c = (int)((idx / ((int64_t)R * R)) % C);
    const int b = (int)(idx / ((int64_t)C * R * R));
    const size_t f = ((size_t)b * R * R + p) * C + c;
    jvp[idx] = fmaf(c_skip[b], vx[idx], c_skip_d[b] * x[idx]) + fmaf(c_out[b], F_d[f], c_out_d[b] * F[f]);
}

}  // namespace

int edm2_launch_attention_mp_jvp(const float* qkv, const float* qkv_d, float* out, float* out_d, int B, int T, int heads, hipStream_t s) {
    if (T % 64 || T <= 0 || heads <= 0 || B <= 0) return (int)hipErrorInvalidValue;  // whole query tiles, whole key tiles
    hipLaunchKernelGGL(edm2_attention_mp_jvp_kernel, dim3(T / 64, heads, B), dim3(NTHR), 0, s, qkv, qkv_d, out, out_d, T, heads);
    RET_LAST();
}

int edm2_launch_pixel_norm_jvp(const float* x, const float* x_d, float* out_d, int B, int H, int C, int down, hipStream_t s) {
    if (B <= 0 || H <= 0 || C <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(edm2_pixel_norm_jvp_kernel, dim3(blocks_for((int64_t)B * H * H, 4)), dim3(256), 0, s, x, x_d, out_d, B, H, C, down);
    RET_LAST();
}

int edm2_launch_silu_operand_jvp(const float* x1, const float* x2, const float* d1, const float* d2, int C1, int C2, const float2* ab,
                                 int ab_stride, const float* ad, int ad_stride, float* out, int B, int64_t hw, hipStream_t s) {
    if (C1 <= 0 || C1 % 4 || C2 < 0 || C2 % 4 || B <= 0 || hw <= 0 || !ab || ab_stride < 0) return (int)hipErrorInvalidValue;
    const int64_t total4 = (int64_t)B * hw * ((C1 + C2) / 4);
    const unsigned grid = (unsigned)std::min<int64_t>((total4 + 255) / 256, 16384);
    hipLaunchKernelGGL(edm2_silu_operand_jvp_kernel, dim3(grid), dim3(256), 0, s, x1, x2, d1, d2, C1, C2, ab, ab_stride, ad, ad_stride, out, hw,
                       total4);
    RET_LAST();
}

int edm2_launch_fourier_jvp(const float* c_noise, const float* c_noise_d, const float* freqs, const float* phases, float* out, int B, int N,
                            hipStream_t s) {
    hipLaunchKernelGGL(edm2_fourier_jvp_kernel, dim3(blocks_for((int64_t)B * N, 256)), dim3(256), 0, s, c_noise, c_noise_d, freqs, phases, out,
                       B, N);
    RET_LAST();
}

int edm2_launch_emb_finish_jvp(const float* e, const float* lab, const float* e_d, float* out, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(edm2_emb_finish_jvp_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, e, lab, e_d, out, n);
    RET_LAST();
}

int edm2_launch_stem_operand_jvp(const float* x_t, const float* vx, const float* c_in, const float* c_in_d, float* out, int B, int C, int R,
                                 int Cp, hipStream_t s) {
    if (Cp < C + 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(edm2_stem_operand_jvp_kernel, dim3(blocks_for((int64_t)B * R * R * Cp, 256)), dim3(256), 0, s, x_t, vx, c_in, c_in_d, out,
                       B, C, R, Cp);
    RET_LAST();
}

int edm2_launch_clamp_jvp(const float* y, float* y_d, float clip, int64_t n, hipStream_t s) {
    if (!(clip > 0.f)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(edm2_clamp_jvp_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, y, y_d, clip, n);
    RET_LAST();
}

int edm2_launch_precond_out_jvp(const float* F, const float* F_d, const float* x_t, const float* vx, const float* c_skip, const float* c_skip_d,
                                const float* c_out, const float* c_out_d, float* jvp, int B, int C, int R, hipStream_t s) {
    hipLaunchKernelGGL(edm2_precond_out_jvp_kernel, dim3(blocks_for((int64_t)B * C * R * R, 256)), dim3(256), 0, s, F, F_d, x_t, vx, c_skip,
                       c_skip_d, c_out, c_out_d, jvp, B, C, R);
    RET_LAST();
}
