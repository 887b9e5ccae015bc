// DhariwalUNet (ADM, reference fastgen/networks/EDM/network.py:584-740) forward kernels: implicit-GEMM convolution with the
// GroupNorm / SiLU prologue, resampling and residual folded in; channel-pair GroupNorm statistics with the adaptive scale / shift
// of UNetBlock(adaptive_scale=True) folded into the coefficients; head-dim-64 attention; the mapping network's input.
// Activations are fp32 NHWC in both compute modes; only the convolution operands are rounded (bf16) or split (bf16x3).
#include "adm.h"
#include "common.h"

#include <math.h>

namespace {

constexpr int NTHR = 256;
constexpr int TM = 128;     // output pixels per workgroup (4 waves x 32)
constexpr int TN = 64;      // output channels per workgroup (2 MFMA column tiles per wave)
constexpr int KC = 32;      // input channels per K-chunk
constexpr int APITCH = 40;  // bf16 per staged pixel row in LDS: 32 + 8 pad (80 bytes: 16-byte aligned fragments)

#define RET_LAST() return (int)hipGetLastError()

// ---------------------------------------------------------------------------------------------------------------------------
// Weight packing: OIHW fp32 -> [Np][taps * Cin] bf16 (K index tap * Cin + ci), lo plane behind the hi plane in the split mode.
__global__ void adm_pack_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int cout, int cin, int taps, int np, int split) {
    const int64_t kp = (int64_t)taps * cin;
    const int64_t total = (int64_t)np * kp;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int n = (int)(e / kp);
        const int k = (int)(e % kp);
        const int tap = k / cin, ci = k % cin;
        const float v = n < cout ? w[((int64_t)n * cin + ci) * taps + tap] : 0.f;
        const __bf16 hi = (__bf16)v;
        out[e] = hi;
        if (split) out[total + e] = (__bf16)(v - (float)hi);
    }
}

// 8 consecutive channels [ch, ch + 8) of source pixel (b, sy, sx) of the virtual concat, fp32
__device__ __forceinline__ void load_src8(const AdmConvArgs& a, int b, int sy, int sx, int ch, float (&v)[8]) {
    const float* p;
    if (ch < a.C1)
        p = a.src1 + (((size_t)b * a.Hs + sy) * a.Hs + sx) * a.C1 + ch;
    else
        p = a.src2 + (((size_t)b * a.Hs + sy) * a.Hs + sx) * a.C2 + (ch - a.C1);
    const f32x4 lo = *reinterpret_cast<const f32x4*>(p);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
    v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
}

__device__ __forceinline__ void pro8(const AdmConvArgs& a, int b, int ch, float (&v)[8]) {
    if (!a.ab) return;
    const float2* ab = a.ab + (size_t)b * (a.ab_stride < 0 ? a.C1 + a.C2 : a.ab_stride) + ch;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float2 k = ab[j];
        const float y = fmaf(v[j], k.x, k.y);
        v[j] = a.silu ? silu_f<false>(y) : y;
    }
}

// Implicit GEMM: M = B*H*H output pixels (TM per workgroup), N = Cout (TN per workgroup), K = taps x Cin in chunks of KC.
// Wave w owns pixels [32w, 32w + 32) of the tile and all TN channels: two 32x32 accumulators.  Per chunk the 128 x 32 operand
// tile is transformed (prologue, resampling) and parked in LDS as bf16 (hi and lo planes in the split mode); the weight
// fragments are read straight from global memory / L2.
template <typename T, int KS>
__global__ __launch_bounds__(NTHR) void adm_conv_kernel(const AdmConvArgs a) {
    constexpr int TAPS = KS * KS;
    constexpr bool X3 = std::is_same<T, bf16x3>::value;
    __shared__ __attribute__((aligned(16))) __bf16 As[X3 ? 2 : 1][TM][APITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, HW = H * H, Cin = a.C1 + a.C2;
    const int M = a.B * HW;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
    const int Np = (a.Cout + TN - 1) / TN * TN;
    const size_t Kp = (size_t)TAPS * Cin;
    const __bf16* wq = reinterpret_cast<const __bf16*>(a.w);

    // staging items: 128 pixels x 4 channel octets, two per thread
    int ib[2], iy[2], ix[2], ipix[2], ioct[2];
    bool iv[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int item = tid + NTHR * r;
        ipix[r] = item >> 2;
        ioct[r] = item & 3;
        const int m = m0 + ipix[r];
        iv[r] = m < M;
        const int mm = iv[r] ? m : 0;
        ib[r] = mm / HW;
        const int rem = mm % HW;
        iy[r] = rem / H;
        ix[r] = rem % H;
    }

    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    const int arow = wave * 32 + (lane & 31), ahalf = lane >> 5;
    for (int tap = 0; tap < TAPS; ++tap) {
        const int dy = KS == 3 ? tap / 3 - 1 : 0, dx = KS == 3 ? tap % 3 - 1 : 0;
        for (int c0 = 0; c0 < Cin; c0 += KC) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                const int uy = iy[r] + dy, ux = ix[r] + dx;
                const int ch = c0 + ioct[r] * 8;
                if (iv[r] && uy >= 0 && uy < H && ux >= 0 && ux < H) {
                    if (a.res_mode == 1) {
                        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            float u[8];
                            load_src8(a, ib[r], 2 * uy + (q >> 1), 2 * ux + (q & 1), ch, u);
                            pro8(a, ib[r], ch, u);
#pragma unroll
                            for (int j = 0; j < 8; ++j) s[j] += u[j];
                        }
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = 0.25f * s[j];
                    } else {
                        const int sy = a.res_mode == 2 ? uy >> 1 : uy, sx = a.res_mode == 2 ? ux >> 1 : ux;
                        load_src8(a, ib[r], sy, sx, ch, v);
                        pro8(a, ib[r], ch, v);
                    }
                }
                __bf16* dst = &As[0][ipix[r]][ioct[r] * 8];
                if (X3) {
                    bf16x8 hi, lo;
                    split8(v, hi, lo);
                    *reinterpret_cast<bf16x8*>(dst) = hi;
                    *reinterpret_cast<bf16x8*>(&As[X3 ? 1 : 0][ipix[r]][ioct[r] * 8]) = lo;
                } else {
                    bf16x8 hi;
#pragma unroll
                    for (int j = 0; j < 8; ++j) hi[j] = (__bf16)v[j];
                    *reinterpret_cast<bf16x8*>(dst) = hi;
                }
            }
            __syncthreads();
            const size_t kg = (size_t)tap * Cin + c0;
#pragma unroll
            for (int kk = 0; kk < KC / 16; ++kk) {
                Frag8<T> af;
                if constexpr (X3) {
                    af.hi = *reinterpret_cast<const bf16x8*>(&As[0][arow][kk * 16 + 8 * ahalf]);
                    af.lo = *reinterpret_cast<const bf16x8*>(&As[X3 ? 1 : 0][arow][kk * 16 + 8 * ahalf]);
                } else {
                    af.v = *reinterpret_cast<const bf16x8*>(&As[0][arow][kk * 16 + 8 * ahalf]);
                }
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const size_t off = (size_t)(n0 + nt * 32 + (lane & 31)) * Kp + kg + kk * 16 + 8 * ahalf;
                    Frag8<T> bf;
                    if constexpr (X3) {
                        bf.hi = *reinterpret_cast<const bf16x8*>(wq + off);
                        bf.lo = *reinterpret_cast<const bf16x8*>(wq + (size_t)Np * Kp + off);
                    } else {
                        bf.v = *reinterpret_cast<const bf16x8*>(wq + off);
                    }
                    mma16(acc[nt], af, bf);
                }
            }
            __syncthreads();
        }
    }

    // epilogue: column (output channel) = lane & 31 of each 32-wide tile, rows = pixels
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int co = n0 + nt * 32 + (lane & 31);
        if (co >= a.Cout) continue;
        const float bo = a.bias ? a.bias[co] : 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = m0 + wave * 32 + acc_row(i, ahalf);
            if (m >= M) continue;
            float v = acc[nt][i] + bo;
            if (a.resid) {
                const int b = m / HW, rem = m % HW, y = rem / H, x = rem % H;
                float r;
                if (a.resid_mode == 0) {
                    r = a.resid[(size_t)m * a.Cout + co];
                } else if (a.resid_mode == 1) {
                    const int R = 2 * H;
                    const float* p = a.resid + (((size_t)b * R + 2 * y) * R + 2 * x) * a.Cout + co;
                    const size_t rs = (size_t)R * a.Cout;
                    r = 0.25f * ((p[0] + p[a.Cout]) + (p[rs] + p[rs + a.Cout]));
                } else {
                    const int R = H / 2;
                    r = a.resid[(((size_t)b * R + (y >> 1)) * R + (x >> 1)) * a.Cout + co];
                }
                if (a.resid_scale != 1.0f) r *= a.resid_scale;
                v += r;
            }
            if (a.clip > 0.0f) v = fminf(fmaxf(v, -a.clip), a.clip);
            a.out[(size_t)m * a.Cout + co] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// GroupNorm, pass 1: part[b][slot][pair] = {sum, sum of squares} over the slot's pixels of channels 2 pair, 2 pair + 1
__global__ __launch_bounds__(NTHR) void adm_gn_part_kernel(const float* __restrict__ x1, int C1, const float* __restrict__ x2, int C2,
                                                           float2* __restrict__ part, int hw, int slots) {
    const int b = blockIdx.x, slot = blockIdx.y;
    const int P = (C1 + C2) / 2;
    const int per = (hw + slots - 1) / slots;
    const int p0 = slot * per, p1 = min(hw, p0 + per);
    for (int q = threadIdx.x; q < P; q += NTHR) {
        const int c = 2 * q;
        const float* base = c < C1 ? x1 + (size_t)b * hw * C1 + c : x2 + (size_t)b * hw * C2 + (c - C1);
        const int stride = c < C1 ? C1 : C2;
        float s = 0.f, ss = 0.f;
        for (int p = p0; p < p1; ++p) {
            const float2 v = *reinterpret_cast<const float2*>(base + (size_t)p * stride);
            s += v.x + v.y;
            ss += v.x * v.x + v.y * v.y;
        }
        part[((size_t)b * slots + slot) * P + q] = make_float2(s, ss);
    }
}

// pass 2: per-group totals in fp64 (fixed order: deterministic), coefficients per channel, adaptive scale / shift folded in
__global__ __launch_bounds__(NTHR) void adm_gn_final_kernel(const float2* __restrict__ part, int C, int slots, int hw,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                            const float* __restrict__ temb, int temb_stride, float2* __restrict__ ab) {
    __shared__ float s_mean[32], s_rstd[32];
    const int b = blockIdx.x;
    const int P = C / 2;
    const int G = min(32, C / 4);
    const int cg = C / G;
    if (threadIdx.x < G) {
        const int g = threadIdx.x;
        double s = 0.0, ss = 0.0;
        for (int sl = 0; sl < slots; ++sl)
            for (int q = g * cg / 2; q < (g + 1) * cg / 2; ++q) {
                const float2 v = part[((size_t)b * slots + sl) * P + q];
                s += v.x;
                ss += v.y;
            }
        const double cnt = (double)cg * hw;
        const double mean = s / cnt;
        double var = ss / cnt - mean * mean;
        if (var < 0.0) var = 0.0;
        s_mean[g] = (float)mean;
        s_rstd[g] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += NTHR) {
        const int g = c / cg;
        float a = s_rstd[g] * gamma[c];
        float bb = fmaf(-a, s_mean[g], beta[c]);
        if (temb) {
            const float sc = 1.0f + temb[(size_t)b * temb_stride + c];
            const float sh = temb[(size_t)b * temb_stride + C + c];
            a *= sc;
            bb = fmaf(bb, sc, sh);
        }
        ab[(size_t)b * C + c] = make_float2(a, bb);
    }
}

int gn_slots(int hw) { return hw >= 128 ? hw / 64 : 1; }

// ---------------------------------------------------------------------------------------------------------------------------
// Attention, head dim 64.  Workgroup = 64 queries of one (image, head); key tiles of 32 streamed through LDS with an online
// softmax (running max / sum per query, output rescaled).  Thread (tq, tk) = (tid / 16, tid % 16) owns queries 4 tq .. 4 tq + 3
// and, for the scores, keys tk + 16 j (j < 2); for the output, dims tk + 16 j (j < 4).  LDS 41 KB.
constexpr int AKT = 32;  // keys per tile

// MP (EDM2) variant: rows [r0, r0 + n) of a [*][pitch] fp32 LDS tile divided by 1e-4 + |row| / 8 (normalize() over 64 channels).
// Four threads per row; n * 4 <= NTHR.
__device__ __forceinline__ void mp_norm_rows(float* tile, int pitch, int n, int tid) {
    const int row = tid >> 2, part = tid & 3;
    float ss = 0.f, inv = 0.f;
    if (row < n) {
        const float* p = tile + (size_t)row * pitch + part * 16;
#pragma unroll
        for (int d = 0; d < 16; ++d) ss = fmaf(p[d], p[d], ss);
    }
    ss += __shfl_xor(ss, 1);
    ss += __shfl_xor(ss, 2);
    __syncthreads();
    if (row < n) {
        inv = 1.0f / (1e-4f + sqrtf(ss) * 0.125f);
        float* p = tile + (size_t)row * pitch + part * 16;
#pragma unroll
        for (int d = 0; d < 16; ++d) p[d] *= inv;
    }
    __syncthreads();
}

template <bool MP>
__global__ __launch_bounds__(NTHR) void adm_attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, int T, int heads) {
    __shared__ float Qs[64][65];                                // [q][d]
    __shared__ float Ks[AKT][65];                               // [k][d], pre-scaled by 1/sqrt(64) = 1/8 (exact)
    __shared__ float Vs[AKT][64];                               // [k][d]
    __shared__ __attribute__((aligned(16))) float Pt[AKT][68];  // [k][q]
    const int tid = threadIdx.x, tq = tid >> 4, tk = tid & 15;
    const int q0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
    const int C = heads * 64, C3 = 3 * C;
    const float* base = qkv + (size_t)b * T * C3 + h * 192;
    for (int e = tid; e < 64 * 64; e += NTHR) {
        const int q = e >> 6, d = e & 63;
        Qs[q][d] = base[(size_t)(q0 + q) * C3 + 3 * d];
    }
    if constexpr (MP) {
        __syncthreads();
        mp_norm_rows(&Qs[0][0], 65, 64, tid);
    }
    float m[4], l[4], o[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m[i] = -INFINITY;
        l[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[i][j] = 0.f;
    }
    for (int k0 = 0; k0 < T; k0 += AKT) {
        for (int e = tid; e < AKT * 64; e += NTHR) {
            const int k = e >> 6, d = e & 63;
            const float* p = base + (size_t)(k0 + k) * C3 + 3 * d;
            Ks[k][d] = MP ? p[1] : p[1] * 0.125f;
            Vs[k][d] = p[2];
        }
        __syncthreads();
        if constexpr (MP) {  // rows 0..31 of Ks, then of Vs; the 1/8 of the logits after the normalisation
            mp_norm_rows(tid < 128 ? &Ks[0][0] : &Vs[0][0], tid < 128 ? 65 : 64, AKT, tid & 127);
            for (int e = tid; e < AKT * 64; e += NTHR) Ks[e >> 6][e & 63] *= 0.125f;
            __syncthreads();
        }
        float s[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i][0] = s[i][1] = 0.f;
#pragma unroll 8
        for (int d = 0; d < 64; ++d) {
            float qv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) qv[i] = Qs[4 * tq + i][d];
            const float k0v = Ks[tk][d], k1v = Ks[tk + 16][d];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[i][0] = fmaf(qv[i], k0v, s[i][0]);
                s[i][1] = fmaf(qv[i], k1v, s[i][1]);
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
            Pt[tk][4 * tq + i] = p0;
            Pt[tk + 16][4 * tq + i] = p1;
            float rs = p0 + p1;
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) rs += __shfl_xor(rs, off);
            l[i] = l[i] * alpha + rs;
            m[i] = mn;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[i][j] *= alpha;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < AKT; ++k) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(&Pt[k][4 * tq]);
            float vv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) vv[j] = Vs[k][tk + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) o[i][j] = fmaf(pv[i], vv[j], o[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float inv = 1.0f / l[i];
        float* dst = out + ((size_t)b * T + q0 + 4 * tq + i) * C + h * 64;
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[tk + 16 * j] = o[i][j] * inv;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ void adm_map_in_kernel(const float* __restrict__ c_noise, const float* __restrict__ freqs, const float* __restrict__ aug,
                                  const float* __restrict__ wa, int aug_dim, float* __restrict__ out, int B, int N) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * N) return;
    const int b = idx / N, j = idx % N, half = N / 2;
    const float ang = c_noise[b] * freqs[j % half];
    float v = j < half ? cosf(ang) : sinf(ang);
    if (aug) {
        float acc = 0.f;
        for (int i = 0; i < aug_dim; ++i) acc = fmaf(aug[(size_t)b * aug_dim + i], wa[(size_t)j * aug_dim + i], acc);
        v += acc;
    }
    out[idx] = v;
}

__global__ void adm_add_silu_kernel(const float* __restrict__ e, const float* __restrict__ lab, float* __restrict__ out, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = silu_f<false>(e[i] + (lab ? lab[i] : 0.f));
}

}  // namespace

size_t adm_conv_pack_elems(int mode, int cout, int cin, int ks) {
    const size_t np = (size_t)(cout + TN - 1) / TN * TN;
    return np * ks * ks * cin * (mode == 2 ? 2 : 1);
}

int adm_pack_conv_weights(int mode, const float* w_oihw, void* out, int cout, int cin, int ks, hipStream_t s) {
    const int np = (cout + TN - 1) / TN * TN;
    const int64_t total = (int64_t)np * ks * ks * cin;
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(adm_pack_kernel, dim3(grid), dim3(256), 0, s, w_oihw, (__bf16*)out, cout, cin, ks * ks, np, mode == 2 ? 1 : 0);
    RET_LAST();
}

int adm_launch_conv(int mode, int ks, const AdmConvArgs& a, hipStream_t s) {
    if ((mode != 1 && mode != 2) || (ks != 1 && ks != 3) || a.C1 % KC || a.C2 % KC || a.C1 + a.C2 == 0 || a.Cout <= 0 || a.B <= 0)
        return (int)hipErrorInvalidValue;
    if ((a.res_mode == 0 && a.Hs != a.H) || (a.res_mode == 1 && a.Hs != 2 * a.H) || (a.res_mode == 2 && 2 * a.Hs != a.H))
        return (int)hipErrorInvalidValue;
    const int64_t M = (int64_t)a.B * a.H * a.H;
    dim3 grid((unsigned)((M + TM - 1) / TM), (unsigned)((a.Cout + TN - 1) / TN));
    if (mode == 2) {
        if (ks == 3) hipLaunchKernelGGL((adm_conv_kernel<bf16x3, 3>), grid, dim3(NTHR), 0, s, a);
        else hipLaunchKernelGGL((adm_conv_kernel<bf16x3, 1>), grid, dim3(NTHR), 0, s, a);
    } else {
        if (ks == 3) hipLaunchKernelGGL((adm_conv_kernel<__bf16, 3>), grid, dim3(NTHR), 0, s, a);
        else hipLaunchKernelGGL((adm_conv_kernel<__bf16, 1>), grid, dim3(NTHR), 0, s, a);
    }
    RET_LAST();
}

size_t adm_gn_part_elems(int B, int hw, int C) { return (size_t)B * gn_slots(hw) * (C / 2); }

int adm_launch_gn(const float* x1, int C1, const float* x2, int C2, const float* gamma, const float* beta, float eps, const float* temb,
                  int temb_stride, float2* part, float2* ab, int B, int hw, hipStream_t s) {
    const int C = C1 + C2;
    if (C < 8 || C1 % 2 || C2 % 2 || (C2 && !x2)) return (int)hipErrorInvalidValue;
    const int G = C / 4 < 32 ? C / 4 : 32;
    if (C % G || (C / G) % 2) return (int)hipErrorInvalidValue;
    const int slots = gn_slots(hw);
    hipLaunchKernelGGL(adm_gn_part_kernel, dim3(B, slots), dim3(NTHR), 0, s, x1, C1, x2, C2, part, hw, slots);
    hipLaunchKernelGGL(adm_gn_final_kernel, dim3(B), dim3(NTHR), 0, s, (const float2*)part, C, slots, hw, gamma, beta, eps, temb,
                       temb_stride, ab);
    RET_LAST();
}

int adm_launch_attention(const float* qkv, float* out, int B, int T, int heads, hipStream_t s) {
    if (T % 64 || T <= 0 || heads <= 0) return (int)hipErrorInvalidValue;  // whole query tiles, whole key tiles
    hipLaunchKernelGGL(adm_attention_kernel<false>, dim3(T / 64, heads, B), dim3(NTHR), 0, s, qkv, out, T, heads);
    RET_LAST();
}

int adm_launch_attention_mp(const float* qkv, float* out, int B, int T, int heads, hipStream_t s) {
    if (T % 64 || T <= 0 || heads <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adm_attention_kernel<true>, dim3(T / 64, heads, B), dim3(NTHR), 0, s, qkv, out, T, heads);
    RET_LAST();
}

int adm_launch_map_in(const float* c_noise, const float* freqs, const float* aug, const float* wa, int aug_dim, float* out, int B, int N,
                      hipStream_t s) {
    hipLaunchKernelGGL(adm_map_in_kernel, dim3((B * N + 255) / 256), dim3(256), 0, s, c_noise, freqs, aug, wa, aug_dim, out, B, N);
    RET_LAST();
}

int adm_launch_add_silu(const float* e, const float* lab, float* out, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(adm_add_silu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, e, lab, out, n);
    RET_LAST();
}
