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
