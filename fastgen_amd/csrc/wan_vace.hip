// VACE (reference fastgen/networks/VaceWan/network.py; diffusers' WanVACETransformer3DModel): the two ends of the control branch.  Its
// hot path is the block kernels of wan.hip / gemm.hip / attn.hip on a second token stream (engine_wan.inc: one block body serves both
// streams); what is new is where that stream begins.  (vace_patch_embedding is wan_embed.hip's plain view with padded output rows.)
//   wan_vace_seed_kernel           c = ctx_in + x0, the control stream's first state (proj_in is applied once per context by
//                                   fg_wan_set_vace_context), one pass with 16-byte accesses
//   wan_vace_scale_rows_kernel      the hint scales as [n][D] fp32 gate rows of the injection GEMM
#include "common.h"
#include "misc.h"

namespace {

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
