// Device primitives the kernel files share beyond common.h's MFMA fragments: wave reductions, small vector types and their
// load / store pairs, the LDS image of the head-dim-128 attention tile, the LDS-only barrier, Philox, the tanh-GELU tangent.
// One definition each: a kernel file that needs one includes this header and adds no copy under a prefix of its own.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) void* lds_ptr;

// ---- 64-lane reductions: every lane ends with the result -----------------------------------------------------------------
// (Two open-coded copies remain, disc.hip logit_kernel and attn_bwd.hip block_reduce: through these functions the compiler orders
// their instructions differently, and this header was introduced under the rule that no kernel's code changes.)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// ---- 2 consecutive activation elements <-> fp32 (the pair form of common.h's load4 / store4) --------------------------------
__device__ __forceinline__ f32x2 load2(const float* p) { return *reinterpret_cast<const f32x2*>(p); }
__device__ __forceinline__ f32x2 load2(const __bf16* p) {
    const bf16x2 q = *reinterpret_cast<const bf16x2*>(p);
    return f32x2{(float)q[0], (float)q[1]};
}
__device__ __forceinline__ void store2(float* p, f32x2 v) { *reinterpret_cast<f32x2*>(p) = v; }
__device__ __forceinline__ void store2(__bf16* p, f32x2 v) { *reinterpret_cast<bf16x2*>(p) = bf16x2{(__bf16)v[0], (__bf16)v[1]}; }

// ---- one token row of the video DiT in one wave: RMSNorm over D = 128 NP (* w; w == nullptr: the row as it is), then (cs_row !=
// nullptr) the interleaved-pair rotation of every head with the token's table row cs_row[64] {cos, sin}.  Lane l holds the pairs
// l + 64 j of the row in v[2 j], v[2 j + 1] (elements 2 (l + 64 j), + 1): register pair j IS head j, pair l of that head.
// Users: wan.hip rms_rope_kernel (bf16 store), wan_kv8.hip wan_kv_quant_kernel (e4m3 store).
template <int NP>
__device__ __forceinline__ void rms_rope_row(const __bf16* __restrict__ x, const float* __restrict__ w, float eps, const float2* __restrict__ cs_row,
                                             int lane, float (&v)[2 * NP]) {
    constexpr int D = 128 * NP;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const bf16x2 q = *reinterpret_cast<const bf16x2*>(x + 2 * (lane + 64 * j));
        v[2 * j] = (float)q[0], v[2 * j + 1] = (float)q[1];
        ss = fmaf(v[2 * j], v[2 * j], fmaf(v[2 * j + 1], v[2 * j + 1], ss));
    }
    if (w) {
        const float r = 1.0f / sqrtf(wave_sum(ss) * (1.0f / D) + eps);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const f32x2 wq = *reinterpret_cast<const f32x2*>(w + 2 * (lane + 64 * j));
            v[2 * j] *= r * wq[0], v[2 * j + 1] *= r * wq[1];
        }
    }
    if (cs_row) {
        const float2 c = cs_row[lane];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const float a = v[2 * j], bb = v[2 * j + 1];
            v[2 * j] = a * c.x - bb * c.y;
            v[2 * j + 1] = a * c.y + bb * c.x;
        }
    }
}

// ---- attention tile, head dim 128: the LDS image----------------------------------------------------------------------------
// A tile is 32 keys x 128 bf16 (8 KiB), for K and for V alike.  V stays row-major in memory and in LDS; its K-contiguous fragments
// (8 keys of one output dim) come from ds_read_b64_tr_b16.  LDS image of both tiles: 256-byte rows, 16-byte chunk ch of row r at
// 16 (ch ^ fa128_swz(r)): conflict-free for the ds_read_b128 row reads of K and for the transposed reads of V
// (cdna_hip_programming.md T10, image (b)).  Users: wan.hip fa_kernel<128> / fa2_kernel (whose LDS-DMA form applies fa128_swz on the
// lane's source address instead), wan_i2v.hip dx_context, wan_jvp.hip wan_attn_jvp_kernel.
__device__ __forceinline__ int fa128_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ int fa128_off(int row, int ch) { return 256 * row + 16 * (ch ^ fa128_swz(row)); }
// the transposed 4 x 16-bit read (generic -> LDS address space: the low 32 bits of a generic LDS pointer are the LDS offset)
__device__ __forceinline__ s16x4 lds_tr_read(const char* lds_addr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)lds_addr);
}

// This wave's LDS traffic retired, then the workgroup barrier.  Deliberately NOT __syncthreads(): its fence would also drain vmcnt
// (weight prefetch rings, epilogue stores and the next tile's loads stay in flight across this one).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Philox4x32-10: counter c -> 4 random words under key (k0, k1).  (misc.hip randn_kernel keeps its own rounds, for the same reason
// as the two reductions above.)
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1, c[3] = (uint32_t)p0, c[0] = n0, c[2] = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// g = gelu_tanh(v) = v sig(2 u), u = sqrt(2/pi) (v + 0.044715 v^3); returns gelu_tanh'(v) = sig + v sig (1 - sig) 2 u',
// u' = sqrt(2/pi) (1 + 3 * 0.044715 v^2).  (The forward-only forms - gemm.hip's gm_gelu_tanh, conv.hip's gelu_tanh_f - are other
// arithmetic: hardware exp2 / rcp.)
__device__ __forceinline__ float gelu_tanh_jvp(float v, float& g) {
    constexpr float c0 = 0.7978845608028654f, c1 = 0.044715f;
    const float v2 = v * v;
    const float u2 = 2.0f * c0 * v * fmaf(c1, v2, 1.0f);
    const float sig = 1.0f / (1.0f + expf(-u2));
    g = v * sig;
    return sig + g * (1.0f - sig) * (2.0f * c0 * fmaf(3.0f * c1, v2, 1.0f));
}
