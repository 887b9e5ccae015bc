// Image-to-video on the bidirectional video DiT (reference fastgen/networks/WanI2V/network.py `WanI2V`, the Wan2.1-I2V convention:
// concat_mask = True, use_image_encoder = True): what that network adds to wan.hip's kernels.  (Its patch embedding of the virtual
// concat [x_t | mask | first_frame_cond] is wan_embed.hip's concat view.)
//   wan_dual_xattn_kernel        cross-attention of an I2V block: softmax(q K_txt^T) V_txt + softmax(q K_img^T) V_img, two independent
//                                online softmaxes (steps 4 + 5 and `hidden_states + hidden_states_img` of Wan/network_causal.py:294-358)
//   wan_ln_rows_kernel           the image embedder's FP32LayerNorm (eps 1e-5, affine) over fp32 or bf16 rows, bf16 out
//   wan_gelu_erf_kernel          its exact (erf) GELU, in place on bf16 (the token GEMM's `act` knows the tanh form only)
// PARITY UNPINNED like the rest of the video DiT: the image branch lives in un-vendored diffusers (WanTimeTextImageEmbedding's
// WanImageEmbedding, WanAttention's add_k_proj / add_v_proj / norm_added_k); tests/wan_i2v_ref.py restates it.
#include "common.h"
#include "../../include/fastgen_amd.h"
#include "misc.h"

namespace {

__device__ __forceinline__ float wsum_i2v(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// fa_kernel<128>'s LDS image (wan.hip): 256-byte rows, 16-byte chunk ch of row r at 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3)))
__device__ __forceinline__ int dx_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

typedef __attribute__((ext_vector_type(4))) short dx_s16x4;
typedef __attribute__((ext_vector_type(8))) short dx_s16x8;
typedef __attribute__((address_space(3))) dx_s16x4 dx_lds_s16x4;
__device__ __forceinline__ dx_s16x4 dx_tr_read(const char* lds_addr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((dx_lds_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)lds_addr);
}

// One context of the dual attention: this wave's 32 queries (fragments qf, the query on the lane) over keys [0, Lkv) of kb / vb,
// normalised, into ot (O^T[dim][query], dims 32 d + acc_row(i, h)).  fa_kernel<128>'s register-staged tile step: 32-key tiles, K and V
// rows double-buffered in LDS (2 x 16 KiB), the next tile's global loads in flight during the current tile, S^T = K Q^T, online
// softmax in the log2 domain, O^T += V^T P^T with transposed V reads.  Key rows are clamped to Lkv - 1 (nothing is read past the
// last key) and masked to -inf in the last tile: they weigh exactly zero.  Every wave of the workgroup calls this (barriers inside).
__device__ __forceinline__ void dx_context(const __bf16* __restrict__ kb, const __bf16* __restrict__ vb, int ldk, int Lkv, const bf16x8 (&qf)[8],
                                           f32x16 (&ot)[4], char* smem, float scale_log2e) {
    constexpr int TILE = 32 * 256, BUF = 2 * TILE;
    const int tid = threadIdx.x, lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    const int gi = lane & 15, gq = gi >> 2, gp = gi & 3, gc = (lane >> 4) & 1;
    fg_u32x4 kreg[2], vreg[2];
    auto issue = [&](int t) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = tid + 256 * i;  // (row p / 16, chunk p % 16) of the tile
            const size_t key = (size_t)min(t * 32 + p / 16, Lkv - 1);
            kreg[i] = *reinterpret_cast<const fg_u32x4*>(kb + key * ldk + (p % 16) * 8);
            vreg[i] = *reinterpret_cast<const fg_u32x4*>(vb + key * ldk + (p % 16) * 8);
        }
    };
    auto park = [&](char* st) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = tid + 256 * i;
            *reinterpret_cast<fg_u32x4*>(st + dx_off(p / 16, p % 16)) = kreg[i];
            *reinterpret_cast<fg_u32x4*>(st + TILE + dx_off(p / 16, p % 16)) = vreg[i];
        }
    };
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) ot[d][i] = 0.f;
    float m = -INFINITY, lsum = 0.f;
    const int ntiles = (Lkv + 31) / 32;
    issue(0);
    park(smem);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const char* st = smem + (t & 1) * BUF;
        if (t + 1 < ntiles) issue(t + 1);
        bf16x8 kf[8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) kf[kk] = *reinterpret_cast<const bf16x8*>(st + dx_off(r, 2 * kk + h));
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kk], qf[kk], s, 0, 0, 0);
        if (t == ntiles - 1) {  // (wave-uniform) only the last key tile can be ragged
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (t * 32 + acc_row(i, h) >= Lkv) s[i] = -INFINITY;
        }
        float mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) mt = fmaxf(mt, s[i]);
        mt = fmaxf(mt, __shfl_xor(mt, 32));  // the other half of the query's keys sits in lane ^ 32
        const float mn = fmaxf(m, mt);       // (finite: the first key of every tile is a real one)
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale_log2e);  // m = -inf at the first tile: exp2(-inf) = 0
        const float mc = mn * scale_log2e;
        float e[16];
        float ps = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            e[i] = __builtin_amdgcn_exp2f(fmaf(s[i], scale_log2e, -mc));
            ps += e[i];  // (the fp32 exponentials are summed before they are rounded for the P V product, as in fa_kernel)
        }
        ps += __shfl_xor(ps, 32);
        lsum = lsum * alpha + ps;
        m = mn;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int i = 0; i < 16; ++i) ot[d][i] *= alpha;
        }
        // O^T[dim][query] += V^T[dim][key] P^T[key][query]: the 16 keys of half sx are accumulator rows 8 sx .. 8 sx + 7 of both lane halves
#pragma unroll
        for (int sx = 0; sx < 2; ++sx) {
            bf16x8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (__bf16)e[8 * sx + j];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int r0 = 16 * sx + 4 * h, c0 = 4 * d + 2 * gc;
                const dx_s16x4 lo = dx_tr_read(st + TILE + dx_off(r0 + gq, c0 + (gp >> 1)) + 8 * (gp & 1));
                const dx_s16x4 hi = dx_tr_read(st + TILE + dx_off(r0 + 8 + gq, c0 + (gp >> 1)) + 8 * (gp & 1));
                const dx_s16x8 vv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                ot[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vv), pf, ot[d], 0, 0, 0);
            }
        }
        if (t + 1 < ntiles) park(smem + ((t + 1) & 1) * BUF);
        __syncthreads();  // tile t + 1 is in LDS; every wave is done with tile t's buffer (tile t + 2 will be parked there)
    }
    const float inv = 1.0f / lsum;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) ot[d][i] *= inv;
}

// grid: 8 ceil(B heads / 8) x ceil(Lq / 128) workgroups of 256 threads, 1-D; a wave owns 32 queries.  All query tiles of one (sample,
// head) run on ONE XCD (workgroup w of a 1-D grid runs on XCD w % 8), as fa_kernel maps them: they read the same K / V rows.
// Q is loaded once, out written once.  THE SUM: each context's normalised output is rounded to bf16, the two are added in fp32 and
// the sum is rounded to bf16 - the reference's arithmetic (two bf16 attention outputs, `hidden_states + hidden_states_img`).  The
// per-element bound of tests/test_gpu_wan_i2v_ops.py therefore carries the term U (A_txt + A_img).  l_img == 0: the text attention
// alone, rounded once.
__global__ __launch_bounds__(256, 2) void wan_dual_xattn_kernel(const __bf16* __restrict__ q, int ldq, int64_t q_bs, const __bf16* __restrict__ k_txt,
                                                                const __bf16* __restrict__ v_txt, int ldk_txt, int64_t kv_bs_txt, int l_txt,
                                                                const __bf16* __restrict__ k_img, const __bf16* __restrict__ v_img, int ldk_img,
                                                                int64_t kv_bs_img, int l_img, __bf16* __restrict__ out, int ldo, int64_t o_bs,
                                                                int Lq, float scale_log2e, int heads, int batch) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int qtiles = (Lq + 127) / 128, units = batch * heads;
    const int xcd = (int)blockIdx.x & 7, slot = (int)blockIdx.x >> 3;
    const int qt = slot % qtiles, unit = (slot / qtiles) * 8 + xcd;
    if (unit >= units) return;  // (the grid is padded to a multiple of 8 units; uniform per workgroup, before any barrier)
    const int head = unit % heads, b = unit / heads;
    const int q0 = qt * 128 + wave * 32;
    // this lane's query row (clamped: rows past Lq compute on the last row and are not stored)
    const __bf16* qrow = q + (size_t)b * q_bs + (size_t)min(q0 + r, Lq - 1) * ldq + head * 128 + 8 * h;
    bf16x8 qf[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(qrow + kk * 16);
    f32x16 ot[4];
    dx_context(k_txt + (size_t)b * kv_bs_txt + head * 128, v_txt + (size_t)b * kv_bs_txt + head * 128, ldk_txt, l_txt, qf, ot, smem, scale_log2e);
    bf16x4 o1[16];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4)
            o1[4 * d + i4] = bf16x4{(__bf16)ot[d][4 * i4], (__bf16)ot[d][4 * i4 + 1], (__bf16)ot[d][4 * i4 + 2], (__bf16)ot[d][4 * i4 + 3]};
    if (l_img > 0) {  // (uniform for the launch)
        dx_context(k_img + (size_t)b * kv_bs_img + head * 128, v_img + (size_t)b * kv_bs_img + head * 128, ldk_img, l_img, qf, ot, smem, scale_log2e);
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4)
#pragma unroll
                for (int e = 0; e < 4; ++e) o1[4 * d + i4][e] = (__bf16)((float)o1[4 * d + i4][e] + (float)(__bf16)ot[d][4 * i4 + e]);
    }
    if (q0 + r < Lq) {
        // out[query][head * 128 + dim]: this lane holds dims 32 d + 8 i4 + 4 h + e of its query
        __bf16* orow = out + (size_t)b * o_bs + (size_t)(q0 + r) * ldo + head * 128;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) *reinterpret_cast<bf16x4*>(orow + 32 * d + 8 * i4 + 4 * h) = o1[4 * d + i4];
    }
}

// One wave per row of n elements: y = (x - mean) * rsqrt(var + eps) * w + b in fp32 (two-pass statistics), bf16 out
template <typename T>
__global__ __launch_bounds__(256) void wan_ln_rows_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                          __bf16* __restrict__ y, int rows, int n, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const T* xr = x + (size_t)row * n;
    float s = 0.f;
    for (int i = lane; i < n; i += 64) s += (float)xr[i];
    const float mean = wsum_i2v(s) / (float)n;
    float ss = 0.f;
    for (int i = lane; i < n; i += 64) {
        const float c = (float)xr[i] - mean;
        ss = fmaf(c, c, ss);
    }
    const float rstd = 1.0f / sqrtf(wsum_i2v(ss) / (float)n + eps);
    for (int i = lane; i < n; i += 64) y[(size_t)row * n + i] = (__bf16)fmaf(((float)xr[i] - mean) * rstd, w[i], b[i]);
}

__global__ void wan_gelu_erf_kernel(__bf16* __restrict__ x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = (float)x[i];
    x[i] = (__bf16)(0.5f * v * (1.0f + erff(v * 0.70710678118654752f)));
}

}  // namespace

int launch_wan_dual_xattn(const void* q, int ldq, int64_t q_bs, const void* k_txt, const void* v_txt, int ldk_txt, int64_t kv_bs_txt, int l_txt,
                          const void* k_img, const void* v_img, int ldk_img, int64_t kv_bs_img, int l_img, void* out, int ldo, int64_t o_bs, int B,
                          int heads, int Lq, hipStream_t s) {
    if ((ldq % 8) || (ldo % 4) || (ldk_txt % 8) || (l_img > 0 && (ldk_img % 8)) || B <= 0 || heads <= 0 || Lq <= 0 || l_txt <= 0 || l_img < 0)
        return (int)hipErrorInvalidValue;
    const long long units = (long long)B * heads;
    const int qtiles = (Lq + 127) / 128;
    const dim3 g((unsigned)(((units + 7) / 8) * 8 * qtiles));
    hipLaunchKernelGGL(wan_dual_xattn_kernel, g, dim3(256), 32768, s, (const __bf16*)q, ldq, q_bs, (const __bf16*)k_txt, (const __bf16*)v_txt, ldk_txt,
                       kv_bs_txt, l_txt, (const __bf16*)k_img, (const __bf16*)v_img, ldk_img, kv_bs_img, l_img, (__bf16*)out, ldo, o_bs, Lq,
                       1.44269504088896341f / sqrtf(128.0f), heads, B);
    return (int)hipGetLastError();
}

int launch_wan_ln_rows(int in_bf16, const void* x, const float* w, const float* b, void* y, int rows, int n, float eps, hipStream_t s) {
    const dim3 g((rows + 3) / 4);
    if (in_bf16) hipLaunchKernelGGL(wan_ln_rows_kernel<__bf16>, g, dim3(256), 0, s, (const __bf16*)x, w, b, (__bf16*)y, rows, n, eps);
    else hipLaunchKernelGGL(wan_ln_rows_kernel<float>, g, dim3(256), 0, s, (const float*)x, w, b, (__bf16*)y, rows, n, eps);
    return (int)hipGetLastError();
}

int launch_wan_gelu_erf(void* x, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(wan_gelu_erf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (__bf16*)x, n);
    return (int)hipGetLastError();
}
