// Kernels of the DhariwalUNet (ADM) forward (adm.hip): fp32 NHWC activations, convolutions as implicit GEMMs on the bf16 matrix
// cores (one product per MFMA in the bf16 mode, the hi/lo split of common.h bf16x3 in the split-bf16 mode), GroupNorm statistics at
// channel-pair granularity with the adaptive scale / shift folded into the coefficients, and head-dim-64 attention with an online
// softmax over streamed key tiles.  All launchers return hipError_t as int.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// y[b, y, x, co] = conv(pro(x))[co] + bias[co] (+ resid[...]), NHWC fp32.
//   input: the virtual concat [src1 (C1) | src2 (C2)] at resolution Hs; res_mode 0: H = Hs, 1: 2x2 mean of the transformed input
//   (H = Hs / 2), 2: nearest 2x replication (H = 2 Hs).  pro: ab == nullptr -> identity, else a*x + b, then SiLU when silu != 0.
//   resid (nullable): Cout channels NHWC; resid_mode 0: same resolution, 1: 2x2 mean of a [2H, 2H] tensor, 2: nearest from [H/2, H/2].
//   EDM2 additions: ab_stride (per-image stride of ab in float2; -1: C1 + C2, 0: one row for every image), resid_scale (the residual
//   enters as resid_scale * resid: mp_sum's skip weight), clip (> 0: the output is clamped to [-clip, clip] after the residual).
struct AdmConvArgs {
    const float* src1 = nullptr;
    const float* src2 = nullptr;
    int C1 = 0, C2 = 0;
    int Hs = 0, H = 0, B = 0;
    int res_mode = 0;
    const float2* ab = nullptr;  // [B][C1 + C2]
    int silu = 0;
    const void* w = nullptr;     // adm_pack_conv_weights layout
    const float* bias = nullptr; // [Cout] or nullptr
    const float* resid = nullptr;
    int resid_mode = 0;
    float* out = nullptr;
    int Cout = 0;
    int ab_stride = -1;
    float resid_scale = 1.0f;
    float clip = 0.0f;
};
// packed weights: [Np][taps * Cin] bf16 (Np = Cout rounded up to 64, rows >= Cout zero), K index = tap * Cin + ci; the split-bf16
// mode stores the lo plane behind the hi plane.  Elements (bf16) of that storage:
size_t adm_conv_pack_elems(int mode, int cout, int cin, int ks);
int adm_pack_conv_weights(int mode, const float* w_oihw, void* out, int cout, int cin, int ks, hipStream_t s);
// mode FG_DTYPE_BF16 (1) or FG_DTYPE_BF16X3 (2); ks 1 or 3.  C1 % 32 == 0, C2 % 32 == 0.
int adm_launch_conv(int mode, int ks, const AdmConvArgs& a, hipStream_t s);

// GroupNorm (groups = min(32, C / 4), biased variance, eps) of the virtual concat [x1 (C1) | x2 (C2)], NHWC fp32 [B, hw, C]:
// ab[b][c] = {a, b} with norm(x) = a x + b.  Two passes: fp32 partial sums per (image, pixel slot, channel pair) into `part`
// (adm_gn_part_elems float2), then per-group fp64 totals.  Group sizes must be even (C1 even).  temb (nullable) folds the
// adaptive scale / shift of UNetBlock(adaptive_scale=True): scale = temb[b * temb_stride + c], shift = temb[b * temb_stride + C + c],
// a' = a (1 + scale), b' = b (1 + scale) + shift.
size_t adm_gn_part_elems(int B, int hw, int C);
int adm_launch_gn(const float* x1, int C1, const float* x2, int C2, const float* gamma, const float* beta, float eps, const float* temb,
                  int temb_stride, float2* part, float2* ab, int B, int hw, hipStream_t s);

// Multi-head self-attention of UNetBlock (EDM/network.py:290-296) with head dim 64: qkv [B, T, 3 C] NHWC as the qkv conv writes it,
// channel h * 192 + 3 c + j (j = q, k, v); out [B, T, C] with channel h * 64 + c.  softmax_k(q . k / 8) in fp32.  T % 64 == 0.
int adm_launch_attention(const float* qkv, float* out, int B, int T, int heads, hipStream_t s);
// EDM2's cosine attention (Block.forward): the same layout, but each of q, k, v is pixel-normalised over its 64 channels on load,
// x / (1e-4 + |x| / 8), before softmax_k(q . k / 8) v.
int adm_launch_attention_mp(const float* qkv, float* out, int B, int T, int heads, hipStream_t s);

// Mapping-network input of DhariwalUNet (EDM/network.py:697-716): [cos | sin] positional embedding of c_noise (endpoint=False,
// no flip) + map_augment(aug) (nullable).  out [B][N].
int adm_launch_map_in(const float* c_noise, const float* freqs, const float* aug, const float* wa, int aug_dim, float* out, int B, int N,
                      hipStream_t s);
// emb = silu(e + lab), lab nullable (= map_label of no labels: zero)
int adm_launch_add_silu(const float* e, const float* lab, float* out, int64_t n, hipStream_t s);
