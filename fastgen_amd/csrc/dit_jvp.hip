// Forward-mode derivative (jvp) of the DiT forward in the split-bf16 mode, 256 tokens (reference
// fastgen/methods/consistency_model/mean_flow.py:220-252: torch.func.jvp through fastgen/networks/DiT/network.py).  A primal stream x
// and a tangent stream xd run side by side, both fp32; the block linears are gemm.hip's split-bf16 token GEMM (launch_gemm_x3: the
// tangent of W a + b is W ad with a null bias).  Here, the pieces that are not GEMMs - each one mirrored in fp64 by
// tests/dit_jvp_ref.py:
//   fourier_jvp_kernel       [cos | sin](t f) and its tangent [-f sin | f cos] td                              (:67-96)
//   silu_jvp_kernel          s = silu(v), sd = silu'(v) (vd_a + vd_b): the embedder MLPs, the adaLN input silu(c)  (:98-101, 186)
//   ln_modulate_jvp_kernel   LayerNorm + adaLN modulation with tangent, both as [hi | lo] planes                (:29-41, 187-196)
//   dit_attention_jvp_kernel softmax(q k^T / sqrt(hd)) v with tangent, per (sample, head), 256 keys' P in registers  (:168, 191)
//   gelu_jvp_kernel          a = gelu_tanh(h), ad = gelu_tanh'(h) hd as planes                                  (:176)
//   gate_update_kernel       x' = x + g h;  xd' += gd h   (xd' arrives as xd + g (W od) from the GEMM's gate + residual epilogue)
//   final_jvp_kernel         OutputProjection + unpatchify of both streams                                        (:218-225, 437-455)
#include "common.h"
#include "misc.h"

namespace {

__device__ __forceinline__ float jv_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ f32x2 jv_ld2(const float* p) { return *reinterpret_cast<const f32x2*>(p); }
typedef __attribute__((ext_vector_type(2))) __bf16 jv_bf16x2;

__global__ void fourier_jvp_kernel(const float* __restrict__ t, const float* __restrict__ td, float* __restrict__ f, float* __restrict__ fd,
                                   int B, int dim) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * dim) return;
    const int b = i / dim, j = i - b * dim, half = dim / 2, jj = j < half ? j : j - half;
    const float freq = expf(-9.210340371976184f * (float)jj / (float)half);
    const float ang = t[b] * freq, c = cosf(ang), s = sinf(ang), d = freq * td[b];
    f[i] = j < half ? c : s;
    fd[i] = j < half ? -s * d : c * d;
}

// s = silu(v) (nullable), sd = silu'(v) (da + db) with silu'(v) = sig (1 + v (1 - sig)); db nullable
__global__ void silu_jvp_kernel(const float* __restrict__ v, const float* __restrict__ da, const float* __restrict__ db, float* __restrict__ s,
                                float* __restrict__ sd, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = v[i], sig = 1.0f / (1.0f + expf(-x));
    float d = da[i];
    if (db) d += db[i];
    if (s) s[i] = x * sig;
    sd[i] = sig * fmaf(x, 1.0f - sig, 1.0f) * d;
}

// One wave per token, lane l holds the channel pairs 2 l + 128 j (ln_modulate_split_kernel's walk).  With n = (x - mu) / sigma:
//   nd = (xd - mean(xd) - n mean(n xd)) / sigma;  y = n (1 + s) + b;  yd = nd (1 + s) + n sd + bd
// mod / modd [B][mod_stride]: shift at shift_off, scale at scale_off, and their tangents at the same places.
template <int D>
__global__ __launch_bounds__(256) void ln_modulate_jvp_kernel(const float* __restrict__ x, const float* __restrict__ xd,
                                                              const float* __restrict__ mod, const float* __restrict__ modd, int mod_stride,
                                                              int shift_off, int scale_off, __bf16* __restrict__ y, __bf16* __restrict__ yd,
                                                              int ntok, int tpi) {
    constexpr int NE = D / 64;
    const int lane = threadIdx.x & 63;
    const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= ntok) return;
    const int n = tok / tpi;
    const float *xrow = x + (size_t)tok * D, *drow = xd + (size_t)tok * D;
    float v[NE], d[NE];
    float s = 0.f, sd = 0.f;
#pragma unroll
    for (int j = 0; j < NE / 2; ++j) {
        const f32x2 q = jv_ld2(xrow + 2 * lane + 128 * j), p = jv_ld2(drow + 2 * lane + 128 * j);
        v[2 * j] = q[0], v[2 * j + 1] = q[1], d[2 * j] = p[0], d[2 * j + 1] = p[1];
        s += q[0] + q[1];
        sd += p[0] + p[1];
    }
    const float mean = jv_wave_sum(s) * (1.0f / D), dmean = jv_wave_sum(sd) * (1.0f / D);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        v[e] -= mean;
        ss = fmaf(v[e], v[e], ss);
    }
    const float rstd = 1.0f / sqrtf(jv_wave_sum(ss) * (1.0f / D) + 1e-6f);
    float nd = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        v[e] *= rstd;
        nd = fmaf(v[e], d[e], nd);
    }
    const float m2 = jv_wave_sum(nd) * (1.0f / D);
    const float *mrow = mod + (size_t)n * mod_stride, *mdrow = modd + (size_t)n * mod_stride;
#pragma unroll
    for (int j = 0; j < NE / 2; ++j) {
        const int c = 2 * lane + 128 * j;
        const f32x2 sc = jv_ld2(mrow + scale_off + c), sh = jv_ld2(mrow + shift_off + c);
        const f32x2 scd = jv_ld2(mdrow + scale_off + c), shd = jv_ld2(mdrow + shift_off + c);
        float o[2], od[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float nn = v[2 * j + e], ndv = (d[2 * j + e] - dmean - nn * m2) * rstd;
            o[e] = fmaf(nn, 1.0f + sc[e], sh[e]);
            od[e] = fmaf(ndv, 1.0f + sc[e], fmaf(nn, scd[e], shd[e]));
        }
        const jv_bf16x2 hi = {(__bf16)o[0], (__bf16)o[1]}, hid = {(__bf16)od[0], (__bf16)od[1]};
        const jv_bf16x2 lo = {(__bf16)(o[0] - (float)hi[0]), (__bf16)(o[1] - (float)hi[1])};
        const jv_bf16x2 lod = {(__bf16)(od[0] - (float)hid[0]), (__bf16)(od[1] - (float)hid[1])};
        *reinterpret_cast<jv_bf16x2*>(y + (size_t)tok * 2 * D + c) = hi;
        *reinterpret_cast<jv_bf16x2*>(y + (size_t)tok * 2 * D + D + c) = lo;
        *reinterpret_cast<jv_bf16x2*>(yd + (size_t)tok * 2 * D + c) = hid;
        *reinterpret_cast<jv_bf16x2*>(yd + (size_t)tok * 2 * D + D + c) = lod;
    }
}

// ---- attention with tangent ---------------------------------------------------------------------------------------------------------
// dit.hip's dit_attention_kernel<bf16x3, HD> (one wave = 32 queries of one (sample, head); S^T = K Q^T with the key on the accumulator
// rows and the query on the lane; all 256 keys' P in registers) carrying a tangent:
//   S = q k^T / sqrt(hd), P = softmax(S), O = P v
//   Sd = (qd k^T + q kd^T) / sqrt(hd), delta_i = sum_j P_ij Sd_ij, Od = (P o (Sd - delta)) v + P vd
// P for all keys AND Sd for all keys are 256 accumulators, which the compiler could not hold without scratch.  So Sd is formed one
// 32-key tile at a time, after the softmax, and consumed at once - with any per-query reference c_i in place of delta_i, since
//   Od_i = sum_j W_ij v_j - (sum_j W_ij) O_i + (P vd)_i,   W_ij = P_ij (Sd_ij - c_i)       (exact for every c_i)
// c_i = the mean of Sd over the first key tile: it removes what is common to a row of Sd (the shift tangent of the modulation reaches
// every key alike and is by far the largest part under scale_t), so W is split into bf16 parts at the size of the result, as
// P o (Sd - delta) would be.  A P fragment feeds O and the P vd term, the k / kd fragments of a tile are shared by both Sd products.
// 128 accumulators for P, 16 for a tile of Sd, 64 / 96 for O and Od, at hd 64 another 64 registers of q and qd fragments: one wave per SIMD
// (launch bound 256 x 1), no scratch.  Operand layouts, the zero-padded 16-deep step of hd 72, the 32 rows of slack and lo_off: as
// dit_attention_kernel.
__device__ __forceinline__ Frag8<bf16x3> jv_planes(const __bf16* p, size_t lo_off, bool valid) {
    Frag8<bf16x3> f;
    f.hi = f.lo = bf16x8{};
    if (valid) {
        f.hi = *reinterpret_cast<const bf16x8*>(p);
        f.lo = *reinterpret_cast<const bf16x8*>(p + lo_off);
    }
    return f;
}
__device__ __forceinline__ Frag8<bf16x3> jv_v_planes(const __bf16* row, size_t lo_off, int key0) {
    Frag8<bf16x3> f;
    const bf16x4 a = *reinterpret_cast<const bf16x4*>(row + key0), b = *reinterpret_cast<const bf16x4*>(row + key0 + 8);
    const bf16x4 c = *reinterpret_cast<const bf16x4*>(row + lo_off + key0), d = *reinterpret_cast<const bf16x4*>(row + lo_off + key0 + 8);
    f.hi = bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    f.lo = bf16x8{c[0], c[1], c[2], c[3], d[0], d[1], d[2], d[3]};
    return f;
}
__device__ __forceinline__ Frag8<bf16x3> jv_pfrag(const f32x16& p, int s) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[8 * s + j];
    Frag8<bf16x3> f;
    split8(v, f.hi, f.lo);
    return f;
}

template <int HD>
__global__ __launch_bounds__(256, 1) void dit_attention_jvp_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                                   const __bf16* __restrict__ vt, const __bf16* __restrict__ qd,
                                                                   const __bf16* __restrict__ kd, const __bf16* __restrict__ vtd,
                                                                   float* __restrict__ out, float* __restrict__ outd, int BH, int heads,
                                                                   size_t lo_off) {
    constexpr int Tn = 256, NT = Tn / 32;
    constexpr int KS = (HD + 15) / 16;
    constexpr int DT_ = (HD + 31) / 32;
    const int lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);  // (sample * heads + head, 32-query slab)
    const int bh = gw / NT, q0 = (gw % NT) * 32;
    if (bh >= BH) return;  // wave-uniform
    const int n = bh / heads, hh = bh - n * heads;

    const size_t qoff = ((size_t)bh * Tn + q0 + r) * HD + 8 * h, koff = ((size_t)bh * Tn + r) * HD + 8 * h;
    // the q / qd fragments stay in registers at hd 64; at hd 72 (80 registers of them) they are read again per key tile, from the
    // cache: with P they have to sit in the 256 architectural registers, and holding them cost 52 bytes of scratch
    constexpr bool HOLD = HD == 64;
    Frag8<bf16x3> qf[KS], qdf[HOLD ? KS : 1];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
        const bool valid = kk * 16 + 8 * h < HD;  // HD % 8 == 0: an 8-element fragment is valid or past the end as a whole
        qf[kk] = jv_planes(q + qoff + kk * 16, lo_off, valid);
        if constexpr (HOLD) qdf[kk] = jv_planes(qd + qoff + kk * 16, lo_off, valid);
    }
    f32x16 st[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) st[kt][i] = 0.f;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
        const bool valid = kk * 16 + 8 * h < HD;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) mma16(st[kt], jv_planes(k + koff + (size_t)kt * 32 * HD + kk * 16, lo_off, valid), qf[kk]);
    }
    // softmax over keys: the other half of this query's logits sits in lane ^ 32
    const float sc = 1.0f / sqrtf((float)HD);
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) m = fmaxf(m, st[kt][i]);
    m = fmaxf(m, __shfl_xor(m, 32));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float e = __builtin_amdgcn_exp2f(1.44269504088896341f * ((st[kt][i] - m) * sc));
            st[kt][i] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) st[kt][i] *= inv;

    // per key tile: Sd, W = P o (Sd - c), then O += P V, Od += W V + P Vd (query on the accumulator row, output dim on the lane)
    const size_t voff = ((size_t)bh * HD + r) * Tn + 4 * h;
    f32x16 o[DT_], od[DT_];
#pragma unroll
    for (int d = 0; d < DT_; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[d][i] = 0.f, od[d][i] = 0.f;
    float cref = 0.f, wsum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        f32x16 w;
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = 0.f;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const bool valid = kk * 16 + 8 * h < HD;
            const size_t ko = koff + (size_t)kt * 32 * HD + kk * 16;
            if constexpr (HOLD) {
                mma16(w, jv_planes(kd + ko, lo_off, valid), qf[kk]);
                mma16(w, jv_planes(k + ko, lo_off, valid), qdf[kk]);
            } else {
                mma16(w, jv_planes(kd + ko, lo_off, valid), jv_planes(q + qoff + kk * 16, lo_off, valid));
                mma16(w, jv_planes(k + ko, lo_off, valid), jv_planes(qd + qoff + kk * 16, lo_off, valid));
            }
        }
        if (kt == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) cref += w[i];
            cref += __shfl_xor(cref, 32);
            cref *= sc * (1.0f / 32.0f);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            w[i] = st[kt][i] * fmaf(w[i], sc, -cref);
            wsum += w[i];
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const Frag8<bf16x3> pf = jv_pfrag(st[kt], s), wf = jv_pfrag(w, s);
#pragma unroll
            for (int d = 0; d < DT_; ++d) {
                const Frag8<bf16x3> vf = jv_v_planes(vt + voff + (size_t)(d * 32) * Tn, lo_off, kt * 32 + 16 * s);
                const Frag8<bf16x3> vdf = jv_v_planes(vtd + voff + (size_t)(d * 32) * Tn, lo_off, kt * 32 + 16 * s);
                mma16(o[d], pf, vf);
                mma16(od[d], wf, vf);
                mma16(od[d], pf, vdf);
            }
        }
    }
    wsum += __shfl_xor(wsum, 32);  // (= delta - c of the lane's query, in both lane halves)
    float wq[16];                  // ... of the queries on this lane's accumulator rows
#pragma unroll
    for (int i = 0; i < 16; ++i) wq[i] = __shfl(wsum, acc_row(i, h));
    const size_t obase = ((size_t)n * Tn + q0) * (heads * HD) + hh * HD + r;
#pragma unroll
    for (int d = 0; d < DT_; ++d)
        if (d * 32 + r < HD) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const size_t at = obase + (size_t)acc_row(i, h) * (heads * HD) + d * 32;
                out[at] = o[d][i];
                outd[at] = fmaf(-wq[i], o[d][i], od[d][i]);
            }
        }
}

// a = gelu_tanh(h) = h sig(2 u), u = sqrt(2/pi) (h + 0.044715 h^3);  ad = (sig + h sig (1 - sig) 2 u') hd,  u' = sqrt(2/pi) (1 + 3 * 0.044715 h^2)
// h, hd fp32 [M][K]; a, ad [hi | lo] planes [M][2 K]; one thread = 4 columns of a row
__global__ __launch_bounds__(256) void gelu_jvp_kernel(const float* __restrict__ h, const float* __restrict__ hd, __bf16* __restrict__ a,
                                                       __bf16* __restrict__ ad, int64_t M, int K) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int K4 = K / 4;
    if (i >= M * K4) return;
    const int64_t r = i / K4;
    const int c = (int)(i - r * K4) * 4;
    const f32x4 x = *reinterpret_cast<const f32x4*>(h + r * K + c), xd = *reinterpret_cast<const f32x4*>(hd + r * K + c);
    bf16x4 hi, lo, hid, lod;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        constexpr float c0 = 0.7978845608028654f, c1 = 0.044715f;
        const float v = x[e], v2 = v * v;
        const float u2 = 2.0f * c0 * v * fmaf(c1, v2, 1.0f);
        const float sig = 1.0f / (1.0f + expf(-u2));
        const float g = v * sig;
        const float gd = (sig + g * (1.0f - sig) * (2.0f * c0 * fmaf(3.0f * c1, v2, 1.0f))) * xd[e];
        hi[e] = (__bf16)g, lo[e] = (__bf16)(g - (float)hi[e]);
        hid[e] = (__bf16)gd, lod[e] = (__bf16)(gd - (float)hid[e]);
    }
    *reinterpret_cast<bf16x4*>(a + r * 2 * K + c) = hi;
    *reinterpret_cast<bf16x4*>(a + r * 2 * K + K + c) = lo;
    *reinterpret_cast<bf16x4*>(ad + r * 2 * K + c) = hid;
    *reinterpret_cast<bf16x4*>(ad + r * 2 * K + K + c) = lod;
}

// xo = x + g h;  xdo += gd h  (g, gd: rows [row / gate_rows] of stride gate_stride; one thread = 4 columns of a row)
__global__ __launch_bounds__(256) void gate_update_kernel(const float* __restrict__ h, const float* __restrict__ g, const float* __restrict__ gd,
                                                          int gate_stride, int gate_rows, const float* __restrict__ x, float* __restrict__ xo,
                                                          float* __restrict__ xdo, int64_t M, int N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int N4 = N / 4;
    if (i >= M * N4) return;
    const int64_t r = i / N4;
    const int c = (int)(i - r * N4) * 4;
    const size_t go = (size_t)(r / gate_rows) * gate_stride + c;
    const f32x4 hv = *reinterpret_cast<const f32x4*>(h + r * N + c);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + go), gdv = *reinterpret_cast<const f32x4*>(gd + go);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + r * N + c), dv = *reinterpret_cast<const f32x4*>(xdo + r * N + c);
    f32x4 a, b;
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = fmaf(gv[e], hv[e], xv[e]), b[e] = fmaf(gdv[e], hv[e], dv[e]);
    *reinterpret_cast<f32x4*>(xo + r * N + c) = a;
    *reinterpret_cast<f32x4*>(xdo + r * N + c) = b;
}

// OutputProjection + unpatchify of both streams (dit.hip final_kernel with the tangent of ln_modulate_jvp_kernel):
// out = b + W y, jvp = W yd;  {shift, scale} = mod[n][0:D], mod[n][D:2D]
template <int D>
__global__ __launch_bounds__(256) void final_jvp_kernel(const float* __restrict__ x, const float* __restrict__ xd, const float* __restrict__ mod,
                                                        const float* __restrict__ modd, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ out, float* __restrict__ outd,
                                                        int ntok, int grid, int p, int C) {
    constexpr int NE = D / 64;
    const int lane = threadIdx.x & 63;
    const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= ntok) return;
    const int tpi = grid * grid, n = tok / tpi, t = tok - n * tpi;
    const float *xrow = x + (size_t)tok * D, *drow = xd + (size_t)tok * D;
    float v[NE], d[NE];
    float s = 0.f, sd = 0.f;
#pragma unroll
    for (int j = 0; j < NE / 2; ++j) {
        const f32x2 q = jv_ld2(xrow + 2 * lane + 128 * j), pp = jv_ld2(drow + 2 * lane + 128 * j);
        v[2 * j] = q[0], v[2 * j + 1] = q[1], d[2 * j] = pp[0], d[2 * j + 1] = pp[1];
        s += q[0] + q[1];
        sd += pp[0] + pp[1];
    }
    const float mean = jv_wave_sum(s) * (1.0f / D), dmean = jv_wave_sum(sd) * (1.0f / D);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        v[e] -= mean;
        ss = fmaf(v[e], v[e], ss);
    }
    const float rstd = 1.0f / sqrtf(jv_wave_sum(ss) * (1.0f / D) + 1e-6f);
    float nd = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        v[e] *= rstd;
        nd = fmaf(v[e], d[e], nd);
    }
    const float m2 = jv_wave_sum(nd) * (1.0f / D);
    const float *mrow = mod + (size_t)n * 2 * D, *mdrow = modd + (size_t)n * 2 * D;
#pragma unroll
    for (int j = 0; j < NE / 2; ++j) {
        const int c = 2 * lane + 128 * j;
        const f32x2 sh = jv_ld2(mrow + c), sc = jv_ld2(mrow + D + c), shd = jv_ld2(mdrow + c), scd = jv_ld2(mdrow + D + c);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float nn = v[2 * j + e], ndv = (d[2 * j + e] - dmean - nn * m2) * rstd;
            v[2 * j + e] = fmaf(nn, 1.0f + sc[e], sh[e]);
            d[2 * j + e] = fmaf(ndv, 1.0f + sc[e], fmaf(nn, scd[e], shd[e]));
        }
    }
    const int PO = p * p * C;
    const int gy = t / grid, gx = t - gy * grid, res = grid * p;
    for (int o = 0; o < PO; ++o) {
        float a = 0.f, ad = 0.f;
#pragma unroll
        for (int j = 0; j < NE / 2; ++j) {
            const f32x2 q = jv_ld2(w + (size_t)o * D + 2 * lane + 128 * j);
            a = fmaf(v[2 * j], q[0], a), a = fmaf(v[2 * j + 1], q[1], a);
            ad = fmaf(d[2 * j], q[0], ad), ad = fmaf(d[2 * j + 1], q[1], ad);
        }
        a = jv_wave_sum(a);
        ad = jv_wave_sum(ad);
        if (lane == 0) {
            const int c = o % C, pq = o / C, py = pq / p, px = pq - py * p;
            const size_t at = (((size_t)n * C + c) * res + gy * p + py) * res + gx * p + px;
            out[at] = a + bias[o];
            outd[at] = ad;
        }
    }
}

#define JVP_RET() return (int)hipGetLastError()

}  // namespace

int launch_dit_fourier_jvp(const float* t, const float* td, float* f, float* fd, int B, int dim, hipStream_t s) {
    hipLaunchKernelGGL(fourier_jvp_kernel, dim3((B * dim + 255) / 256), dim3(256), 0, s, t, td, f, fd, B, dim);
    JVP_RET();
}
int launch_dit_silu_jvp(const float* v, const float* da, const float* db, float* sout, float* sd, int n, hipStream_t s) {
    hipLaunchKernelGGL(silu_jvp_kernel, dim3((n + 255) / 256), dim3(256), 0, s, v, da, db, sout, sd, n);
    JVP_RET();
}
int launch_dit_ln_modulate_jvp(int D, const float* x, const float* xd, const float* mod, const float* modd, int mod_stride, int shift_off,
                               int scale_off, void* y, void* yd, int ntok, int tokens_per_image, hipStream_t s) {
    if (ntok <= 0 || tokens_per_image <= 0 || (mod_stride % 2) || (shift_off % 2) || (scale_off % 2)) return (int)hipErrorInvalidValue;  // (8-byte loads)
    dim3 g((ntok + 3) / 4), b(256);
#define LNJ(DD) hipLaunchKernelGGL((ln_modulate_jvp_kernel<DD>), g, b, 0, s, x, xd, mod, modd, mod_stride, shift_off, scale_off, (__bf16*)y, (__bf16*)yd, ntok, tokens_per_image)
    switch (D) {
        case 384: LNJ(384); break;
        case 768: LNJ(768); break;
        case 1024: LNJ(1024); break;
        case 1152: LNJ(1152); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef LNJ
    JVP_RET();
}
int launch_dit_attention_jvp(const void* q, const void* k, const void* vt, const void* qd, const void* kd, const void* vtd, float* out, float* outd,
                             int B, int heads, int head_dim, int T, size_t lo_off, hipStream_t s) {
    const int64_t BH = (int64_t)B * heads;
    if (T != 256 || (head_dim != 64 && head_dim != 72) || B <= 0 || heads <= 0 || BH * 8 > INT32_MAX) return (int)hipErrorInvalidValue;
    dim3 g((unsigned)(BH * 2)), b(256);  // 8 slabs of 32 queries per (sample, head), 4 waves per workgroup
#define ATJ(HD) hipLaunchKernelGGL((dit_attention_jvp_kernel<HD>), g, b, 0, s, (const __bf16*)q, (const __bf16*)k, (const __bf16*)vt, (const __bf16*)qd, \
                                   (const __bf16*)kd, (const __bf16*)vtd, out, outd, (int)BH, heads, lo_off)
    if (head_dim == 72) ATJ(72);
    else ATJ(64);
#undef ATJ
    JVP_RET();
}
int launch_dit_gelu_jvp(const float* h, const float* hd, void* a, void* ad, int64_t M, int K, hipStream_t s) {
    if (M <= 0 || K <= 0 || (K % 4) || (M * (K / 4) + 255) / 256 > INT32_MAX) return (int)hipErrorInvalidValue;
    const int64_t n = M * (K / 4);
    hipLaunchKernelGGL(gelu_jvp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h, hd, (__bf16*)a, (__bf16*)ad, M, K);
    JVP_RET();
}
int launch_dit_gate_update(const float* h, const float* g, const float* gd, int gate_stride, int gate_rows, const float* x, float* xo, float* xdo,
                           int64_t M, int N, hipStream_t s) {
    if (M <= 0 || N <= 0 || (N % 4) || (gate_stride % 4) || gate_rows <= 0 || (M * (N / 4) + 255) / 256 > INT32_MAX) return (int)hipErrorInvalidValue;
    const int64_t n = M * (N / 4);
    hipLaunchKernelGGL(gate_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h, g, gd, gate_stride, gate_rows, x, xo, xdo, M, N);
    JVP_RET();
}
int launch_dit_final_jvp(int D, const float* x, const float* xd, const float* mod, const float* modd, const float* w, const float* bias, float* out,
                         float* outd, int ntok, int grid, int p, int C, hipStream_t s) {
    dim3 g((ntok + 3) / 4), b(256);
#define FNJ(DD) hipLaunchKernelGGL((final_jvp_kernel<DD>), g, b, 0, s, x, xd, mod, modd, w, bias, out, outd, ntok, grid, p, C)
    switch (D) {
        case 384: FNJ(384); break;
        case 768: FNJ(768); break;
        case 1024: FNJ(1024); break;
        case 1152: FNJ(1152); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef FNJ
    JVP_RET();
}
