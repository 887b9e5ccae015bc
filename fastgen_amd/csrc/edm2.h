// Kernels of the EDM2 U-Net forward (edm2.hip) besides the shared ADM convolution and attention (adm.h): magnitude-preserving weight
// preparation, pixel norm, the MP-Fourier embedding and its finish, the per-block modulation rows, the stem operand and the output
// preconditioning.  fp32 NHWC activations.  All launchers return hipError_t as int.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// MPConv's forward weight (normalize, then the magnitude-preserving scale) with extra folds, as an fp32 OIHW (or [O][I]) copy whose
// input channels are zero-padded to cin_pad:
//   out[o][ci][tap] = w[o][ci][tap] * (gain ? *gain : 1) * extra[ci < c_split ? 0 : 1] / sqrt(fan_in) / (1e-4 + |w_o| / sqrt(fan_in))
// with fan_in = cin * taps.  gain: device scalar (emb_gain / out_gain) or nullptr.  c_split >= cin: extra[0] for every column.
int edm2_launch_prep_weight(const float* w, float* out, int cout, int cin, int cin_pad, int taps, const float* gain, float extra0,
                            float extra1, int c_split, hipStream_t s);

// Pixel norm x / (1e-4 + |x| / sqrt(C)) over the channels of every pixel, NHWC [B, H, H, C] -> same shape; down != 0: the input is
// [B, 2H, 2H, C] and is averaged over 2x2 first (resample 'down' with f = [1, 1]).  In place is allowed when down == 0.
int edm2_launch_pixel_norm(const float* x, float* out, int B, int H, int C, int down, hipStream_t s);

// MPFourier: out[b][j] = cos(c_noise[b] * freqs[j] + phases[j]) * sqrt(2), fp32.
int edm2_launch_fourier(const float* c_noise, const float* freqs, const float* phases, float* out, int B, int N, hipStream_t s);

// mp_silu(e + lab) = silu(e + lab) / 0.596 (lab nullable).
int edm2_launch_emb_finish(const float* e, const float* lab, float* out, int64_t n, hipStream_t s);

// ab[i] = {1 + c[i], 0}: the conv_res1 prologue rows silu(c * y) of every block from the stacked emb_linear outputs.
int edm2_launch_mod_rows(const float* c, float2* ab, int64_t n, hipStream_t s);

// Stem operand: NHWC [B, R, R, Cp] with channels [c_in[b] * x_t (C, NCHW) | 1 | 0 ...].
int edm2_launch_stem_operand(const float* x_t, const float* c_in, float* out, int B, int C, int R, int Cp, hipStream_t s);

// precond_output: out[b, c, y, x] (NCHW) = c_skip[b] x_t[b, c, y, x] + c_out[b] F[b, y, x, c] (F NHWC with C channels).
int edm2_launch_precond_out(const float* F, const float* x_t, const float* c_skip, const float* c_out, float* out, int B, int C, int R,
                            hipStream_t s);

// ---- forward-mode derivative (edm2_jvp.hip): tangents `_d` beside the primal values the forward kernels read or wrote ---------------

// jvp of adm_launch_attention_mp in one pass over the keys: qkv, qkv_d [B, T, 3 C] in that launcher's layout; out_d (and out, nullable:
// the primal, bit-equal to adm_launch_attention_mp) [B, T, C].  Each q, k, v row x with n = 1e-4 + |x| / 8: x^ = x / n,
// x^_d = x_d / n - x (x . x_d) / (8 |x| n^2) (0 where |x| = 0); s = q^ . k^ / 8, s_d = (q^_d . k^ + q^ . k^_d) / 8;
// O_d = sum_k p (s_d v^ + v^_d) / l - (sum_k p s_d / l) O.  Head dim 64, T % 64 == 0.
int edm2_launch_attention_mp_jvp(const float* qkv, const float* qkv_d, float* out, float* out_d, int B, int T, int heads, hipStream_t s);

// jvp of edm2_launch_pixel_norm: x, x_d at the source resolution (2H with down != 0: both are averaged over 2x2 first), out_d
// [B, H, H, C] = m_d / n - m (m . m_d) / (sqrt(C) |m| n^2), n = 1e-4 + |m| / sqrt(C) (m_d / 1e-4 where m = 0).  out_d may be x_d when
// down == 0.
int edm2_launch_pixel_norm_jvp(const float* x, const float* x_d, float* out_d, int B, int H, int C, int down, hipStream_t s);

// The tangent convolution's operand behind a SiLU prologue: out [B, hw, C1 + C2] = silu'(a x + b) (a x_d + a_d x) over the virtual
// concat [x1 | x2] (tangents d1 | d2), {a, b} = ab[img * ab_stride + c] (ab_stride 0: one row for every image), a_d = ad ?
// ad[img * ad_stride + c] : 0.  The tangent convolution is then adm_launch_conv on `out` with ab = nullptr and the primal's weights.
// C1 % 4 == 0, C2 % 4 == 0.
int edm2_launch_silu_operand_jvp(const float* x1, const float* x2, const float* d1, const float* d2, int C1, int C2, const float2* ab,
                                 int ab_stride, const float* ad, int ad_stride, float* out, int B, int64_t hw, hipStream_t s);

// MPFourier tangent: out[b][j] = -sqrt(2) sin(c_noise[b] freqs[j] + phases[j]) freqs[j] c_noise_d[b].
int edm2_launch_fourier_jvp(const float* c_noise, const float* c_noise_d, const float* freqs, const float* phases, float* out, int B, int N,
                            hipStream_t s);

// Tangent of edm2_launch_emb_finish: out = silu'(e + lab) / 0.596 * e_d (lab nullable; the label embedding has no tangent).
int edm2_launch_emb_finish_jvp(const float* e, const float* lab, const float* e_d, float* out, int64_t n, hipStream_t s);

// Tangent of the stem operand: NHWC [B, R, R, Cp] with channels [c_in[b] vx + c_in_d[b] x_t (C, NCHW) | 0 | 0 ...].
int edm2_launch_stem_operand_jvp(const float* x_t, const float* vx, const float* c_in, const float* c_in_d, float* out, int B, int C, int R,
                                 int Cp, hipStream_t s);

// Tangent of the convolution's clamp, in place: y_d = 0 where the clamped primal output has |y| >= clip.  torch.clamp passes the
// tangent where the pre-clamp value equals +-clip exactly; this zeroes it there (a set of measure zero).
int edm2_launch_clamp_jvp(const float* y, float* y_d, float clip, int64_t n, hipStream_t s);

// Tangent of edm2_launch_precond_out: jvp (NCHW) = c_skip vx + c_skip_d x_t + c_out F_d + c_out_d F (F, F_d NHWC).
int edm2_launch_precond_out_jvp(const float* F, const float* F_d, const float* x_t, const float* vx, const float* c_skip, const float* c_skip_d,
                                const float* c_out, const float* c_out_d, float* jvp, int B, int C, int R, hipStream_t s);
