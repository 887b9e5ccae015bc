// Causal video DiT: the self-attention K / V cache stored as e4m3fn bytes (fg_wan_set_kv_cache_dtype(h, FG_DTYPE_FP8)), head dim 128.
// The cache halves; the arithmetic does not change: bytes are widened back to bf16 (exact: e4m3 has 3 mantissa bits) in front of the
// same v_mfma_f32_32x32x16_bf16 products fa_kernel<128> issues, so given the stored values the result is the bf16 kernel's.
//   cache     K, V  [B][Lcache] rows of ld bytes (head hd at byte 128 hd), one fp32 scale per (token, head): [B][Lcache][H]
//   wan_kv_quant_kernel   the cache write: token.h's rms_rope_row (RMSNorm * weight, RoPE - the arithmetic of rms_rope_kernel) with a
//                         quantising tail: per (token, head) amax over its 128 dims, scale = amax / 448 (zero head: scale 1, bytes 0),
//                         bytes = common.h's fp8_pack4 (the row quantiser's clamp + v_cvt_pk_fp8_f32).
//                         LANE MAP: one wave per token; lane l holds elements 2 l, 2 l + 1 of EVERY head - head j is register pair j -
//                         so a head's amax is a 64-lane wave_max of max(|v[2 j]|, |v[2 j + 1]|), a wave stores the 128 bytes of a head
//                         as 64 two-byte lanes, and lane j stores head j's scale.
//   wan_fa_kv8_kernel     softmax(q k^T / sqrt(128)) v of bf16 queries over cache rows [0, Lkv).
//
// wan_fa_kv8_kernel.  Grid: fa_kernel's (a (sample, head) unit lives on one XCD, its query tiles side by side); workgroup = 4 waves =
// 128 queries, a wave owns 32.  The transposed form of fa_kernel: S^T = K Q^T (key on the accumulator row, QUERY on the lane),
// O^T = V^T P^T (output dim on the row, query on the lane) - m, l and the rescale factor of a query are one lane's scalars (its keys'
// other half sits in lane ^ 32).  Keys go by tiles of 64 = two 32-key S^T blocks; a tile's K bytes, V bytes and 2 x 64 scales travel
// global -> registers -> LDS once per workgroup, two LDS buffers, the loads of tile t + 1 issued before tile t's MFMAs.
// Rows past Lkv are never read (the staging clamps the key index, the logits of the clamped copies are masked).
//
// The contraction slots of an MFMA may be any 16 dims / keys as long as both operands agree, which is what makes byte tiles cheap:
//   K tile    row-major [64 keys][128 B], pitch 144.  Lane (key r, half h) reads its row's bytes 64 h .. 64 h + 63 as four
//             ds_read_b128; step kk of q k^T contracts dims 64 h + 8 kk .. + 7 (8 bytes of those 16 dwords), and the lane's Q fragment
//             kk is loaded from the same dims.  144 = 9 x 16: the 16 rows of a 16-lane group fall on 16 different 16-byte slots of
//             the 256-byte bank window (9 r mod 16 is a permutation) - conflict-free.
//   V tile    TRANSPOSED while it is parked: [128 dims][64 keys], pitch 80.  A staging thread loads a 4 keys x 4 dims block (four
//             dwords), transposes it with eight v_perm_b32 and writes one dword (4 consecutive keys) per dim.  Inside a dim's row the
//             key quad g = key / 4 sits at dword 8 (g & 1) + (g >> 1): lane (dim r, half h) then finds ALL its keys of the tile -
//             32 b + 8 j + 4 h + e, exactly the keys whose P^T it meets (acc_row) - in bytes 32 h .. 32 h + 31, two ds_read_b128;
//             dwords 2 s, 2 s + 1 are the operand of PV step s = 2 b + (j >> 1).  80 = 5 x 16: conflict-free as above (5 r mod 16).
//             (The transposing dword writes collide 8-way - dims 4 apart are 320 bytes apart; 8 writes per thread and tile.)
//   scales    ks[64] | vs[64] fp32 per buffer; a lane reads the four scales of accumulator rows 4 j .. 4 j + 3 as one b128
//             (a broadcast: every lane of a half reads the same address).
// The K scale multiplies the logit row of its key behind the S^T product; the V scale multiplies P of its key in front of P's
// rounding to bf16 (the row sum l takes the unscaled P); P is never normalised, O is divided by l once.
// LDS: 2 x (9216 + 10240 + 512) = 39 936 bytes: two workgroups per CU.
#include <type_traits>

#include "token.h"
#include "../../include/fastgen_amd.h"
#include "misc.h"

namespace {

template <int NP>
__global__ __launch_bounds__(256) void wan_kv_quant_kernel(const __bf16* __restrict__ src, int ld_src, const float* __restrict__ w, float eps,
                                                           const float2* __restrict__ cs, unsigned char* __restrict__ dst,
                                                           float* __restrict__ scale, int64_t dst_bs, int64_t scale_bs, int dst_row0, int ld_dst,
                                                           int rows, int L) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = row / L, l = row - b * L;
    float v[2 * NP];
    rms_rope_row<NP>(src + (size_t)row * ld_src, w, eps, cs ? cs + (size_t)l * 64 : nullptr, lane, v);
    unsigned char* y = dst + (size_t)b * dst_bs + (size_t)(dst_row0 + l) * ld_dst;
    float mine = 0.f;  // head `lane`'s scale
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const float amax = wave_max(fmaxf(fabsf(v[2 * j]), fabsf(v[2 * j + 1])));
        // (a zero head: zero bytes, not the rotation's -0)
        const unsigned q = amax == 0.f ? 0u : fp8_pack4(f32x4{v[2 * j], v[2 * j + 1], 0.f, 0.f}, fp8_row_inv(amax));
        *reinterpret_cast<unsigned short*>(y + 128 * j + 2 * lane) = (unsigned short)q;
        mine = lane == j ? fp8_row_scale(amax) : mine;
    }
    if (lane < NP) scale[(size_t)b * scale_bs + (size_t)(dst_row0 + l) * NP + lane] = mine;
}

// 8 e4m3fn bytes -> 8 bf16 (v_cvt_scalef32_pk_bf16_fp8 at scale 1: exact)
__device__ __forceinline__ bf16x8 kv8_widen(unsigned lo, unsigned hi) {
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
    return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

constexpr int KV8_KP = 144, KV8_VP = 80;                   // LDS pitches of the K tile / the transposed V tile
constexpr int KV8_VOFF = 64 * KV8_KP;                      // V tile behind the K tile
constexpr int KV8_SOFF = KV8_VOFF + 128 * KV8_VP;          // ks[64] | vs[64]
constexpr int KV8_BUF = KV8_SOFF + 128 * (int)sizeof(float);

__global__ __launch_bounds__(256, 2) void wan_fa_kv8_kernel(const __bf16* __restrict__ q, int ldq, int64_t q_bs, const unsigned char* __restrict__ k8,
                                                            const unsigned char* __restrict__ v8, int ldk, int64_t kv_bs,
                                                            const float* __restrict__ k_scale, const float* __restrict__ v_scale, int64_t scale_bs,
                                                            __bf16* __restrict__ out, int ldo, int64_t o_bs, int Lq, int Lkv, float scale_log2e,
                                                            int heads, int batch) {
    __shared__ __attribute__((aligned(16))) char smem[2 * KV8_BUF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    // workgroup -> ((sample, head) unit, query tile): fa_kernel's map
    const int qtiles = (Lq + 127) / 128, units = batch * heads;
    const int xcd = (int)blockIdx.x & 7, slot = (int)blockIdx.x >> 3;
    const int qt = slot % qtiles, unit = (slot / qtiles) * 8 + xcd;
    if (unit >= units) return;  // (the grid is padded to a multiple of 8 units; uniform per workgroup, before any barrier)
    const int head = unit % heads, b = unit / heads;
    const int q0 = qt * 128 + wave * 32;
    // this lane's query row (clamped: rows past Lq compute on the last row and are not stored), dims 64 h + 8 kk .. + 7 per step
    const __bf16* qrow = q + (size_t)b * q_bs + (size_t)min(q0 + r, Lq - 1) * ldq + head * 128 + 64 * h;
    bf16x8 qf[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(qrow + 8 * kk);
    const unsigned char* kb = k8 + (size_t)b * kv_bs + head * 128;
    const unsigned char* vb = v8 + (size_t)b * kv_bs + head * 128;
    const float* sb = (tid < 64 ? k_scale : v_scale) + (size_t)b * scale_bs + head;  // (threads 0 .. 127 stage the scales)

    // staging registers of one tile: K as 2 x 16 bytes (row p / 8, chunk p % 8), V as 2 blocks of 4 keys (quad g) x 4 dims (quad dq)
    const int dq = tid & 31;
    fg_u32x4 kreg[2];
    unsigned vreg[2][4];
    float sreg = 0.f;
    auto issue = [&](int t) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = tid + 256 * i;
            const size_t key = (size_t)min(t * 64 + (p >> 3), Lkv - 1);
            kreg[i] = *reinterpret_cast<const fg_u32x4*>(kb + key * ldk + (p & 7) * 16);
            const int g = (tid >> 5) + 8 * i;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                vreg[i][e] = *reinterpret_cast<const unsigned*>(vb + (size_t)min(t * 64 + 4 * g + e, Lkv - 1) * ldk + 4 * dq);
        }
        if (tid < 128) sreg = sb[(size_t)min(t * 64 + (tid & 63), Lkv - 1) * heads];
    };
    auto park = [&](char* st) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = tid + 256 * i;
            *reinterpret_cast<fg_u32x4*>(st + (p >> 3) * KV8_KP + (p & 7) * 16) = kreg[i];
            // 4 x 4 byte transpose: x / y = keys (0, 1) / (2, 3) interleaved per dim, then the dim's four keys
            const unsigned xl = __builtin_amdgcn_perm(vreg[i][1], vreg[i][0], 0x05010400u), xh = __builtin_amdgcn_perm(vreg[i][1], vreg[i][0], 0x07030602u);
            const unsigned yl = __builtin_amdgcn_perm(vreg[i][3], vreg[i][2], 0x05010400u), yh = __builtin_amdgcn_perm(vreg[i][3], vreg[i][2], 0x07030602u);
            const unsigned tr[4] = {__builtin_amdgcn_perm(yl, xl, 0x05040100u), __builtin_amdgcn_perm(yl, xl, 0x07060302u),
                                    __builtin_amdgcn_perm(yh, xh, 0x05040100u), __builtin_amdgcn_perm(yh, xh, 0x07060302u)};
            const int g = (tid >> 5) + 8 * i;
            char* vt = st + KV8_VOFF + 4 * (8 * (g & 1) + (g >> 1));
#pragma unroll
            for (int c = 0; c < 4; ++c) *reinterpret_cast<unsigned*>(vt + (4 * dq + c) * KV8_VP) = tr[c];
        }
        if (tid < 128) reinterpret_cast<float*>(st + KV8_SOFF)[tid] = sreg;
    };

    f32x16 ot[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) ot[d][i] = 0.f;
    float m = -INFINITY, lsum = 0.f;
    const int ntiles = (Lkv + 63) / 64;

    auto step = [&](int t, auto BI_) {
        constexpr int BI = decltype(BI_)::value;  // tile t sits in buffer BI
        const char* st = smem + BI * KV8_BUF;
        if (t + 1 < ntiles) issue(t + 1);
        const float* ks = reinterpret_cast<const float*>(st + KV8_SOFF);
        const float* vs = ks + 64;
        // S^T[key][query] of the tile's two 32-key blocks, each logit row times its key's scale
        f32x16 s[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            fg_u32x4 kw[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) kw[c] = *reinterpret_cast<const fg_u32x4*>(st + (32 * blk + r) * KV8_KP + 64 * h + 16 * c);
#pragma unroll
            for (int i = 0; i < 16; ++i) s[blk][i] = 0.f;
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
                s[blk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kv8_widen(kw[kk >> 1][2 * (kk & 1)], kw[kk >> 1][2 * (kk & 1) + 1]), qf[kk], s[blk], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 sc = *reinterpret_cast<const f32x4*>(ks + 32 * blk + 8 * j + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[blk][4 * j + e] *= sc[e];
            }
        }
        // online softmax; keys past Lkv (last tile) are masked
        if (t == ntiles - 1) {  // (wave-uniform) only the last key tile can be ragged
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (t * 64 + 32 * blk + acc_row(i, h) >= Lkv) s[blk][i] = -INFINITY;
        }
        float mt = -INFINITY;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int i = 0; i < 16; ++i) mt = fmaxf(mt, s[blk][i]);
        mt = fmaxf(mt, __shfl_xor(mt, 32));  // the other half of the query's keys sits in lane ^ 32
        const float mn = fmaxf(m, mt);
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale_log2e);  // m = -inf at the first tile: exp2(-inf) = 0
        const float mc = mn * scale_log2e;
        float ps = 0.f;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s[blk][i] = __builtin_amdgcn_exp2f(fmaf(s[blk][i], scale_log2e, -mc));
                ps += s[blk][i];
            }
        ps += __shfl_xor(ps, 32);
        lsum = lsum * alpha + ps;
        m = mn;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {  // wave-uniform: the running maximum of some query of this wave moved
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int i = 0; i < 16; ++i) ot[d][i] *= alpha;
        }
        // P^T fragments: step sx = 2 blk + (j >> 1) takes accumulator rows 8 (sx & 1) .. + 7 of block blk, each times its key's V scale
        bf16x8 pf[4];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 sc = *reinterpret_cast<const f32x4*>(vs + 32 * blk + 8 * j + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) pf[2 * blk + (j >> 1)][4 * (j & 1) + e] = (__bf16)(s[blk][4 * j + e] * sc[e]);
            }
        // O^T[dim][query] += V^T[dim][key] P^T[key][query]
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const fg_u32x4 v0 = *reinterpret_cast<const fg_u32x4*>(st + KV8_VOFF + (32 * d + r) * KV8_VP + 32 * h);
            const fg_u32x4 v1 = *reinterpret_cast<const fg_u32x4*>(st + KV8_VOFF + (32 * d + r) * KV8_VP + 32 * h + 16);
            ot[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kv8_widen(v0[0], v0[1]), pf[0], ot[d], 0, 0, 0);
            ot[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kv8_widen(v0[2], v0[3]), pf[1], ot[d], 0, 0, 0);
            ot[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kv8_widen(v1[0], v1[1]), pf[2], ot[d], 0, 0, 0);
            ot[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kv8_widen(v1[2], v1[3]), pf[3], ot[d], 0, 0, 0);
        }
        if (t + 1 < ntiles) park(smem + (1 - BI) * KV8_BUF);  // (its readers passed the barrier that ended tile t - 1)
        __syncthreads();
    };
    issue(0);
    park(smem);
    __syncthreads();
    for (int t = 0; t < ntiles; t += 2) {
        step(t, std::integral_constant<int, 0>{});
        if (t + 1 < ntiles) step(t + 1, std::integral_constant<int, 1>{});
    }
    // out[query][head * 128 + dim]: this lane holds dims 32 d + acc_row(i, h) = 32 d + 8 i4 + 4 h + e of its query
    if (q0 + r < Lq) {
        const float inv = 1.0f / lsum;
        __bf16* orow = out + (size_t)b * o_bs + (size_t)(q0 + r) * ldo + head * 128;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) {
                const bf16x4 o4 = {(__bf16)(ot[d][4 * i4] * inv), (__bf16)(ot[d][4 * i4 + 1] * inv), (__bf16)(ot[d][4 * i4 + 2] * inv),
                                   (__bf16)(ot[d][4 * i4 + 3] * inv)};
                *reinterpret_cast<bf16x4*>(orow + 32 * d + 8 * i4 + 4 * h) = o4;
            }
    }
}

}  // namespace

// launch_rms_rope's operands with an e4m3 destination: dst rows of ld_dst bytes, dst_bs bytes between samples; scale [B][scale_bs]
// floats, row (dst_row0 + l) of a sample at (dst_row0 + l) * (D / 128).  D: one of misc.h's FG_WAN_WIDTHS.
int launch_wan_kv_quant(int D, const void* src, int ld_src, const float* w, float eps, const float2* cs, void* dst, float* scale, int64_t dst_bs,
                        int64_t scale_bs, int dst_row0, int ld_dst, int rows, int L, hipStream_t s) {
    dim3 g((rows + 3) / 4), b(256);
    if (!fg_wan_width_call(D, [&](auto d) {
            hipLaunchKernelGGL(wan_kv_quant_kernel<decltype(d)::value / 128>, g, b, 0, s, (const __bf16*)src, ld_src, w, eps, cs, (unsigned char*)dst,
                               scale, dst_bs, scale_bs, dst_row0, ld_dst, rows, L);
        }))
        return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

int launch_wan_fa_kv8(const void* q, int ldq, int64_t q_bs, const void* k8, const void* v8, int ldk, int64_t kv_bs, const float* k_scale,
                      const float* v_scale, int64_t scale_bs, void* out, int ldo, int64_t o_bs, int B, int heads, int Lq, int Lkv, hipStream_t s) {
    if (B <= 0 || heads <= 0 || Lq <= 0 || Lkv <= 0) return (int)hipErrorInvalidValue;
    const int64_t grid = (((int64_t)B * heads + 7) / 8) * 8 * ((Lq + 127) / 128);
    if (grid > INT32_MAX) return (int)hipErrorInvalidValue;
    const float scale_log2e = 1.4426950408889634f / sqrtf(128.0f);
    hipLaunchKernelGGL(wan_fa_kv8_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const __bf16*)q, ldq, q_bs, (const unsigned char*)k8,
                       (const unsigned char*)v8, ldk, kv_bs, k_scale, v_scale, scale_bs, (__bf16*)out, ldo, o_bs, Lq, Lkv, scale_log2e, heads, B);
    return (int)hipGetLastError();
}
