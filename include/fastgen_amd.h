/*
 * fastgen_amd — C ABI of the MI355X-native few-step diffusion sampling path (libfastgen_amd.so).
 *
 * Drop-in boundary for ONE hot path of the reference (paths relative to the reference repo root):
 *     FastGenModel.generator_fn / _student_sample_loop      fastgen/methods/model.py:315-420
 *       -> EDMPrecond.forward -> SongUNet.forward             fastgen/networks/EDM/network.py:881-974, 489-574
 *       -> EDMNoiseSchedule.{latents,forward_process,x0_to_eps}  fastgen/networks/noise_schedule.py:72-88,425-449,544-574
 *
 * Everything here is plain C: opaque handle, raw device pointers, sizes, an explicit HIP stream
 * (passed as void* = hipStream_t).  No torch types.  All functions return 0 on success and a
 * non-zero FG_E* code on failure; fg_last_error() returns a thread-local message.  A handle is
 * re-entrant per stream only in the sense that calls on ONE handle must be serialised by the
 * caller (one Python thread per process in the reference).
 *
 * Tensors at the boundary keep the reference's layout and dtype: images are fp32 NCHW [B,C,H,W],
 * timesteps are fp64 [B] (noise_schedule.py:41,50), class labels fp32 [B,label_dim], parameters
 * are fp32 in the reference's state-dict shapes (OIHW conv weights).  Internally activations are
 * NHWC and weights are re-packed into MFMA fragment order; that never leaks through this ABI.
 */
#ifndef FASTGEN_AMD_H
#define FASTGEN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Every entry point below is exported with default visibility; nothing else leaves the library (it is built with
 * -fvisibility=hidden). */
#define FG_API __attribute__((visibility("default")))

#define FG_OK 0
#define FG_EINVAL 1      /* bad argument / unsupported configuration */
#define FG_ENOTREADY 2   /* a parameter is unbound or weights were not packed */
#define FG_EHIP 3        /* a HIP runtime call failed (message holds hipGetErrorString) */
#define FG_ENOMEM 4      /* workspace too small */

#define FG_DTYPE_F32 0   /* exact fp32: v_mfma_f32_32x32x2_f32, fp32 activations */
#define FG_DTYPE_BF16 1  /* bf16 MFMA operands, fp32 accumulate, bf16 activation storage, fp32 norm statistics / softmax */
/* Split-bf16 convolutions on fp32 tensors: every conv operand x is split into hi = bf16(x), lo = bf16(x - hi) and a product is
 * a_lo*b_hi + a_hi*b_lo + a_hi*b_hi on the bf16 matrix pipe with fp32 accumulate (about 2^-17 relative per product, against
 * 2^-11 for the TF32 arithmetic the reference enables on NVIDIA GPUs, fastgen/utils/scripts.py:43-45, which gfx950 does not have);
 * activations, statistics, attention, embedding MLP and preconditioning exactly as FG_DTYPE_F32.  Three bf16 MFMAs per product:
 * roofline 2.5 PFLOP/s / 3, against 157 TFLOP/s for FG_DTYPE_F32. */
#define FG_DTYPE_BF16X3 2
/* fp8 (the DiT and the causal video DiT): the linears of every transformer block - the DiT's four, the video DiT's six (fg_wan_config)
 * - contract OCP e4m3fn operands (W8A8, v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales, fp32 accumulate): weights quantised
 * per output channel at pack time, activations per token on every call (scale = amax / 448, q = RNE(clamp(x * (448 / amax), -448,
 * 448))); everything else - token tensors, attention, embeddings, the modulation GEMM, the final layer - exactly as FG_DTYPE_BF16.
 * hidden_size and mlp_hidden (ffn_dim) must be multiples of 128.  Roofline 5 PFLOP/s.  The EDM / EDM2 / ADM handles refuse it. */
#define FG_DTYPE_FP8 3

#define FG_SAMPLE_SDE 0  /* student_sample_type='sde'  (methods/model.py:358-359) */
#define FG_SAMPLE_ODE 1  /* student_sample_type='ode'  (methods/model.py:360-361) */

#define FG_LOOP_X0 0        /* FastGenModel._student_sample_loop: x0 prediction + re-noise (methods/model.py:315-372) */
#define FG_LOOP_MEANFLOW 1  /* MeanFlowModel._student_sample_loop: x -= dt * u(x,t,r) (consistency_model/mean_flow.py:336-381) */
#define FG_LOOP_EULER 2     /* DiT._sample_flow: Euler steps of the flow ODE, optional classifier-free guidance (DiT/network.py:605-651);
                               fg_dit_sampler_run only */

#define FG_SCHEDULE_EDM 0   /* EDMNoiseSchedule: alpha = 1, sigma = t, t in [0.002, 80] (noise_schedule.py:729-777) */
#define FG_SCHEDULE_RF 1    /* RFNoiseSchedule:  alpha = 1 - t, sigma = t, t in [0, 0.999] (noise_schedule.py:1306-1341) */

#define FG_DROP_PRECOND_INPUT 1   /* drop_precond 'input'  (EDM/network.py:929-934); 'both' = INPUT | OUTPUT */
#define FG_DROP_PRECOND_OUTPUT 2  /* drop_precond 'output' (EDM/network.py:959-960) */

#define FG_MAX_LEVELS 8

/* fg_edm_config.model_type: the U-Net inside EDMPrecond (EDM/network.py:830-836). */
#define FG_MODEL_SONGUNET 0  /* DDPM++ (SongUNet, :322-574): everything below unless stated otherwise */
/* ADM (DhariwalUNet, :584-740; configs/net.py:50-66, the ImageNet-64 teacher): adaptive-scale blocks with GroupNorm eps 1e-5,
 * skip_scale 1, 64-channel attention heads, a [cos | sin] noise embedding and a bias-free map_label added after map_layer1.
 * Forward and sampling only: fg_edm_create / param_info / bind / pack / workspace_bytes / fg_edm_forward / fg_sampler_run.
 * fg_edm_num_blocks / fg_edm_block_info / fg_edm_run_block serve its UNetBlocks (below); the feature taps, backward, jvp and
 * training entry points return FG_EINVAL on such a handle.  compute_dtype
 * FG_DTYPE_BF16X3 or FG_DTYPE_BF16 (activations stay fp32 in both); r_timestep 0; img_resolution 8 .. 64; every level's width
 * a multiple of 64; attention at 8x8 .. 32x32.  cfg.channel_mult_noise is ignored (cond_channels = model_channels). */
#define FG_MODEL_DHARIWAL 1

/* kwargs of EDMPrecond(model_type="SongUNet", embedding_type="positional", encoder_type=decoder_type="standard",
 * resample_filter=[1,1], dropout=0) — fastgen/configs/net.py:29-48 and EDM/network.py:347-367, 809-821. */
typedef struct fg_edm_config {
    int img_resolution;                  /* 32 */
    int img_channels;                    /* 3 */
    int label_dim;                       /* 10 (0 = unconditional) */
    int augment_dim;                     /* 9: map_augment exists in the state dict but is skipped when sampling */
    int model_channels;                  /* 128 */
    int num_levels;                      /* len(channel_mult) */
    int channel_mult[FG_MAX_LEVELS];     /* {2,2,2} */
    int channel_mult_emb;                /* 4 */
    int num_blocks;                      /* 4 */
    int num_attn_resolutions;
    int attn_resolutions[FG_MAX_LEVELS]; /* {16} */
    int channel_mult_noise;              /* 1 */
    double sigma_data;                   /* 0.5 */
    double sigma_shift;                  /* 0.0 (applied in eval mode only, EDM/network.py:956: see fg_edm_set_training) */
    int compute_dtype;                   /* FG_DTYPE_* */
    int r_timestep;                      /* 1: second (target-time) embedding, cond_channels doubled (EDM/network.py:376,401-408) */
    int drop_precond;                    /* bit mask of FG_DROP_PRECOND_* (0 = full EDM preconditioning) */
    int schedule;                        /* FG_SCHEDULE_*: the noise schedule the sampler loop re-noises with */
    int model_type;                      /* FG_MODEL_*: 0 (a zero-initialised config) = SongUNet */
} fg_edm_config;

typedef struct fg_edm fg_edm; /* opaque */

/* Thread-local message of the last failing call on this thread ("" if none). */
FG_API const char* fg_last_error(void);
/* "fastgen_amd <version> gfx950" */
FG_API const char* fg_version(void);
/* Process-wide, read-only counts of the sampler entry points' hipGraph work (either pointer may be null): `captures` graphs
 * instantiated (a use_graph call whose cached graph did not match its arguments), `launches` graphs launched.  A replay is a launch
 * without a capture: launches - captures.  Read the two before and after a call and take the differences. */
FG_API void fg_graph_stats(uint64_t* captures, uint64_t* launches);

/* ---- network object: replaces EDMPrecond.__init__ / state-dict ownership (EDM/network.py:808-839) ---- */
FG_API int fg_edm_create(const fg_edm_config* cfg, fg_edm** out);
FG_API void fg_edm_destroy(fg_edm* h);

/* State-dict view: the entries of the reference's EDMPrecond.state_dict() that carry weights (parameters
 * only; the constant resample_filter buffers are folded into the kernels).  Same names, same shapes. */
FG_API int fg_edm_num_params(const fg_edm* h);
FG_API int fg_edm_param_info(const fg_edm* h, int index, const char** name, int* ndim, int64_t shape[4]);

/* Bind a parameter to caller-owned DEVICE memory (fp32, reference layout).  The pointer is borrowed: it is
 * read again by every fg_edm_pack_weights() and must stay valid until then.  Used instead of a one-shot
 * load so FSDP2 / optimizer updates can re-bind and re-pack. */
FG_API int fg_edm_bind_param(fg_edm* h, const char* name, const float* device_ptr, int64_t numel);
/* Build the kernel-layout copies (MFMA fragment order, compute dtype) of all bound parameters. */
FG_API int fg_edm_pack_weights(fg_edm* h, void* stream);

/* Bytes of caller-provided scratch needed for a batch (activations, skip stack, norm statistics ...). */
FG_API size_t fg_edm_workspace_bytes(const fg_edm* h, int batch);

/* EDMPrecond.forward(x_t, t, condition=class_labels, r=r, fwd_pred_type=net_pred_type) in eval mode
 * (EDM/network.py:881-974).  x_t,out: [B,C,H,W] fp32; t: [B] fp64; r: [B] fp64, required iff cfg.r_timestep (else
 * NULL, :505-510); class_labels: [B,label_dim] fp32 or NULL (NULL = the reference's zeros([1,label_dim]) broadcast,
 * :919-925).  All device pointers.  x_t is not modified; out may not alias x_t.  emb_out (nullable):
 * [B, model_channels*channel_mult_emb] mapping-network output. */
FG_API int fg_edm_forward(fg_edm* h, const float* x_t, const double* t, const double* r, const float* class_labels, float* out,
                   float* emb_out, int batch, void* workspace, size_t workspace_bytes, void* stream);

/* The same forward with the encoder feature taps of SongUNet.forward (EDM/network.py:525-544, 562-567): tap i is the i-th
 * encoder block whose name contains "block3" (the last block of resolution level i for num_blocks = 4), the tensors the
 * DMD2 discriminator reads (methods/distribution_matching/dmd2.py:142).  features: HOST array of
 * fg_edm_num_feature_taps() device pointers, each NULL (not requested: the reference's feature_indices set) or an
 * [B, channels, res, res] fp32 NCHW buffer.  out == NULL is return_features_early: the decoder is not run. */
FG_API int fg_edm_num_feature_taps(const fg_edm* h);
FG_API int fg_edm_feature_info(const fg_edm* h, int index, const char** key, int* channels, int* resolution);
FG_API int fg_edm_forward_features(fg_edm* h, const float* x_t, const double* t, const double* r, const float* class_labels,
                            float* out, float* const* features, int batch, void* workspace, size_t workspace_bytes,
                            void* stream);

/* FastGenModel.generator_fn (methods/model.py:374-420) around one of the student sampling loops:
 *   x = noise * sigma(t_list[0]);
 *   FG_LOOP_X0 (model.py:315-372, x0-predicting network without r_timestep):
 *     for i: x0 = forward(x, t_i); if t_{i+1} > 0: x = alpha(t_{i+1}) x0 + sigma(t_{i+1}) eps_i; return x0
 *     ('ode': eps_i = x0_to_eps(x, x0, t_i)).
 *   FG_LOOP_MEANFLOW (mean_flow.py:336-381, flow-predicting r_timestep network):
 *     'sde': x -= t_i * forward(x, t_i, r=0); if t_{i+1} > 0: x = forward_process(x, eps_i, t_{i+1});
 *     'ode': x -= (t_i - t_{i+1}) * forward(x, t_i, r=t_{i+1});   return x.
 * t_list: HOST array of steps+1 doubles, steps in [1, 64], t_list[steps] must be 0 (model.py:410) and every other entry inside
 * the schedule's [min_t, max_t] up to one fp32 ulp (is_t_valid, noise_schedule.py:409-423: float32 lists pass).  sample_type
 * FG_SAMPLE_*.  These checks, shared by every *_sampler_run, come before the handle's state: FG_EINVAL before FG_ENOTREADY.
 * eps: device [steps-1][B,C,H,W] noise to inject in 'sde' mode, or NULL to draw it on device from
 * (seed, step) with Philox4x32-10.  use_graph != 0 replays a cached hipGraph of the whole loop. */
FG_API int fg_sampler_run(fg_edm* h, const float* noise, const float* class_labels, const double* t_list, int steps,
                   int sample_type, int loop_kind, const float* eps, uint64_t seed, float* out, int batch,
                   void* workspace, size_t workspace_bytes, int use_graph, void* stream);

/* EDMNoiseSchedule.get_t_list(sample_steps) (noise_schedule.py:940-973) -> steps+1 doubles on the host. */
FG_API int fg_edm_t_list(int sample_steps, double* out_host);
/* RFNoiseSchedule.get_t_list(sample_steps) = BaseNoiseSchedule.get_t_list (noise_schedule.py:259-272). */
FG_API int fg_rf_t_list(int sample_steps, double* out_host);

/* ---- measurement hook (bench.py): time every launch of the dominant kernel — the fused 3x3 conv at 32x32 output
 * without resampling — with a hipEvent pair on the stream it is launched on.  While active the sampler runs eagerly
 * (no graph replay).  profile_end() synchronises the events and returns launches, summed milliseconds and summed
 * algorithmic FLOPs (2 * B*H*W * Cout * 9*Cin per launch). */
FG_API int fg_edm_profile_begin(fg_edm* h);
FG_API int fg_edm_profile_end(fg_edm* h, int64_t* launches, double* total_ms, double* total_flops);

/* ---- single-op entry points (used by the parity tests; same kernels the network path launches) ---- */

/* One UNetBlock (EDM/network.py:274-299) by index into the encoder+decoder block list.  Inputs NHWC fp32:
 * x1 [B,Hin,Win,c1] (+ optional x2 [B,Hin,Win,c2] = the skip tensor of the decoder's channel concat),
 * emb [B,emb_channels]; out [B,H,W,cout] NHWC. */
FG_API int fg_edm_num_blocks(const fg_edm* h);
FG_API int fg_edm_block_info(const fg_edm* h, int index, const char** key, int* cin, int* cout, int* res_in, int* res_out,
                      int* has_attention);
FG_API int fg_edm_run_block(fg_edm* h, int index, const float* x1, int c1, const float* x2, int c2, const float* emb,
                     float* out, int batch, void* workspace, size_t workspace_bytes, void* stream);
/* On an FG_MODEL_DHARIWAL handle the list is the encoder's UNetBlocks, then the decoder's (the stem and the output head are not
 * blocks); key "model.enc.<res>x<res>_<name>" / "model.dec...."; res_in = 2 res_out for a down block, res_out / 2 for an up block.
 * A decoder block's c2 is its skip width (cin minus the previous block's cout), 0 elsewhere; any other c1 / c2 split is FG_EINVAL. */

/* GroupNorm statistics folded with the affine parameters: ab[b][c] = {a, b} with y = a*x + b
 * (GroupNorm.forward, EDM/network.py:141-149; groups = min(32, C/4)).  x NHWC fp32 [B,HW,C]. */
FG_API int fg_op_gn_coeffs(const float* x1, int c1, const float* x2, int c2, const float* gamma, const float* beta,
                    float eps, float* ab_out, int batch, int hw, void* stream);

/* ---- DhariwalUNet single-op entry points: the kernels fg_edm_forward runs on an FG_MODEL_DHARIWAL handle (fp32 NHWC tensors).
 * Arguments are checked before anything is launched: a bad shape, mode or pointer is FG_EINVAL. */
/* Convolution weights OIHW fp32 [cout][cin][ks][ks] -> the operand of fg_op_adm_conv.  mode FG_DTYPE_BF16 or FG_DTYPE_BF16X3 (hi and
 * lo bf16 planes), ks 1 or 3, cin % 32 == 0.  _bytes: size of `packed`, 0 for an unsupported argument. */
FG_API size_t fg_op_adm_conv_pack_bytes(int mode, int cout, int cin, int ks);
FG_API int fg_op_adm_conv_pack(int mode, const float* w_oihw, void* packed, int cout, int cin, int ks, void* stream);
/* out[b,y,x,co] = conv_ks(R(pro(x)))[co] + bias[co] (+ resid) with zero padding.  x = the channel concat [src1 (c1) | src2 (c2)]
 * at resolution hs, c1 > 0 and c2 >= 0 multiples of 32; ab (nullable) [batch][c1 + c2] {a, b}: pro(x) = a x + b, then SiLU when
 * silu != 0.  R: res_mode 0 identity (h = hs), 1 2x2 mean (hs = 2 h), 2 nearest 2x (h = 2 hs).  bias nullable.  resid
 * (nullable) [batch][.][.][cout]: resid_mode 0 at h, 1 the 2x2 mean of a 2h tensor, 2 nearest from h / 2.  out [batch][h][h][cout].
 * src1 / src2 / packed 16-byte aligned. */
FG_API int fg_op_adm_conv(int mode, int ks, const float* src1, int c1, const float* src2, int c2, int batch, int hs, int h,
                          int res_mode, const float* ab, int silu, const void* packed, const float* bias, const float* resid,
                          int resid_mode, float* out, int cout, void* stream);
/* fg_op_adm_conv with the three EDM2 fields of the kernel.  ab_stride: the per-image stride of ab in {a, b} pairs: -1 = c1 + c2 (dense
 * rows, fg_op_adm_conv), 0 = one row [c1 + c2] for every image, >= c1 + c2 = rows inside a wider matrix (ab points at the first image's
 * first channel); anything else is FG_EINVAL.  resid_scale (finite): the residual enters as resid_scale * resid (one fp32 product, then
 * the sum).  clip (finite, >= 0): > 0 clamps the output to [-clip, clip] AFTER the residual; 0 = no clamp.
 * fg_op_adm_conv is this call with (-1, 1.0f, 0.0f). */
FG_API int fg_op_adm_conv_ex(int mode, int ks, const float* src1, int c1, const float* src2, int c2, int batch, int hs, int h,
                             int res_mode, const float* ab, int ab_stride, int silu, const void* packed, const float* bias,
                             const float* resid, int resid_mode, float resid_scale, float clip, float* out, int cout, void* stream);
/* GroupNorm (groups = min(32, C / 4), C = c1 + c2 even-sized groups, c1 / c2 even) of the concat [x1 | x2], NHWC [batch][hw][C]:
 * ab_out[b][c] = {a, b} with norm(x) = a x + b; temb (nullable, row stride temb_stride >= 2C) folds the adaptive scale / shift:
 * a (1 + temb[c]), b (1 + temb[c]) + temb[C + c].  workspace: fg_op_adm_gn_workspace_bytes (0: unsupported). */
FG_API size_t fg_op_adm_gn_workspace_bytes(int batch, int hw, int c);
FG_API int fg_op_adm_gn_coeffs(const float* x1, int c1, const float* x2, int c2, const float* gamma, const float* beta, float eps,
                               const float* temb, int temb_stride, float* ab_out, int batch, int hw, void* workspace,
                               size_t workspace_bytes, void* stream);
/* Self-attention with head dim 64: qkv [batch][t][heads * 192], channel h * 192 + 3 c + j (j = q, k, v); out [batch][t][heads * 64]
 * = softmax_k(q . k / 8) v.  t % 64 == 0. */
FG_API int fg_op_adm_attention(const float* qkv, float* out, int batch, int t, int heads, void* stream);
/* ---- EDM2 single-op entry points and the shared linear (used by the parity tests: the kernels fg_edm2_forward runs).  Arguments are
 * checked before anything is launched: a bad shape or pointer is FG_EINVAL. */
/* EDM2's cosine attention: fg_op_adm_attention's layout and checks; each of q, k, v is divided by 1e-4 + |.| / 8 over its 64 channels
 * before softmax_k(q . k / 8) v. */
FG_API int fg_op_edm2_attention(const float* qkv, float* out, int batch, int t, int heads, void* stream);
/* MPConv's forward weight with the folds of fg_edm2_pack_weights: w [cout][cin][taps] -> out [cout][cin_pad][taps] (cin_pad >= cin, the
 * padding columns zero), out[o][ci][tap] = w[o][ci][tap] * g * (ci < c_split ? extra0 : extra1) / sqrt(fan) / (1e-4 + |w_o| / sqrt(fan)),
 * fan = cin * taps, g = *gain (a device scalar) or 1 when gain is NULL.  out must not alias w. */
FG_API int fg_op_edm2_prep_weight(const float* w, float* out, int cout, int cin, int cin_pad, int taps, const float* gain, float extra0,
                                  float extra1, int c_split, void* stream);
/* Pixel norm x / (1e-4 + |x| / sqrt(c)) over the channels of every pixel, NHWC: down == 0: x, out [batch][h][h][c], out == x allowed;
 * down == 1: x [batch][2h][2h][c] is averaged over 2x2 first (out must not alias x). */
FG_API int fg_op_edm2_pixel_norm(const float* x, float* out, int batch, int h, int c, int down, void* stream);
/* ---- EDM2 tangent kernels (the ones fg_edm2_jvp runs beside the forward's), same checks.  `_d` is a tangent. */
/* jvp of fg_op_edm2_attention in one pass over the keys: qkv_d in qkv's layout, out_d [batch][t][heads * 64]; out (nullable) receives
 * the primal, bit-equal to fg_op_edm2_attention.  Row x with n = 1e-4 + |x| / 8: x^_d = x_d / n - x (x . x_d) / (8 |x| n^2), 0 where
 * |x| = 0. */
FG_API int fg_op_edm2_attention_jvp(const float* qkv, const float* qkv_d, float* out, float* out_d, int batch, int t, int heads, void* stream);
/* jvp of fg_op_edm2_pixel_norm: with down == 1 both x and x_d are averaged over 2x2 first.  out_d == x_d allowed with down == 0. */
FG_API int fg_op_edm2_pixel_norm_jvp(const float* x, const float* x_d, float* out_d, int batch, int h, int c, int down, void* stream);
/* The tangent convolution's operand behind a SiLU prologue, out [batch][hw][c1 + c2] = silu'(a x + b) (a x_d + a_d x) over the virtual
 * concat [x1 | x2] (tangents d1 | d2): {a, b} = ab[2 * (img * ab_stride + c)] (float pairs; ab_stride 0: one row for every image),
 * a_d = ad ? ad[img * ad_stride + c] : 0.  c1, c2 multiples of 4; tensors 16-byte aligned. */
FG_API int fg_op_edm2_silu_operand_jvp(const float* x1, const float* x2, const float* d1, const float* d2, int c1, int c2, const float* ab,
                                       int ab_stride, const float* ad, int ad_stride, float* out, int batch, int hw, void* stream);
/* y [batch][out] = act(x [batch][in] w[out][in]^T + bias): the linear layer of all four engines (embeddings, modulations).  bias nullable;
 * act_silu != 0: SiLU after the bias.  Shapes with in % 16 == 0 and out % 32 == 0 run on the fp32 matrix pipe with 16-byte loads: there
 * x and w must be 16-byte aligned (FG_EINVAL otherwise; the engines' buffers always are).  Every other shape runs the FMA kernel, which
 * has no alignment requirement.  y must not alias x. */
FG_API int fg_op_linear(const float* x, const float* w, const float* bias, float* y, int batch, int in, int out, int act_silu, void* stream);
/* Mapping-network input: out[b] = [cos | sin](c_noise[b] * freqs) (+ wa aug[b] when aug != nullptr), freqs [n / 2], wa [n][aug_dim],
 * out [batch][n], n even. */
FG_API int fg_op_adm_map_in(const float* c_noise, const float* freqs, const float* aug, const float* wa, int aug_dim, float* out,
                            int batch, int n, void* stream);

/* Elementwise sampler steps in fp64 (noise_schedule.py:72-88, 425-449, 544-574); n = elements per sample. */
FG_API int fg_op_latents(const float* noise, double t_init, float* out, int64_t total, void* stream);
FG_API int fg_op_forward_process(const float* x0, const float* eps, double t, int schedule, float* out, int64_t total,
                          void* stream);
FG_API int fg_op_x0_to_eps(const float* xt, const float* x0, double t, int schedule, float* out, int64_t total, void* stream);
/* ---- training step, first kernel (forward-only sampling does not use it) --------------------------------
 * Weight gradient of Conv2d.forward (EDM/network.py:93-126) as autograd computes it in the DMD2 student / fake-score
 * updates: dw[co][ci][ky][kx] (+)= sum_{n,y,x} dy[n,y,x,co] * act[n,y+ky-ks/2,x+kx-ks/2,ci], zero padding.
 * act [B,res,res,cin] and dy [B,res,res,cout] are NHWC bf16 (the conv's input operand and its output gradient),
 * dw is fp32 OIHW [cout,cin,ks,ks]; accumulate != 0 adds to dw.  Deterministic (fixed-order split-K reduction through
 * the workspace).  res in {8,16,32}, cin % 32 == 0 (ks = 3) / cin % 128 == 0 (ks = 1), cout % 128 == 0, ks in {1,3}. */
FG_API size_t fg_op_conv_wgrad_workspace_bytes(int batch, int res, int cin, int cout, int ks);
FG_API int fg_op_conv_wgrad(const void* act, const void* dy, float* dw, int batch, int res, int cin, int cout, int ks,
                     int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* The same weight gradient in the split-bf16 compute mode (FG_DTYPE_BF16X3): act and dy are NHWC fp32, each split into hi / lo
 * bf16 planes on the way into LDS, dy_lo*a_hi + dy_hi*a_lo + dy_hi*a_hi with fp32 accumulation.  Same shapes, workspace size
 * (fg_op_conv_wgrad_workspace_bytes) and determinism. */
FG_API int fg_op_conv_wgrad_f32(const float* act, const float* dy, float* dw, int batch, int res, int cin, int cout, int ks,
                                int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of one UNetBlock (EDM/network.py:274-299) as autograd computes it (bf16 or bf16x3 compute mode; every block variant: attention,
 * 2x down / up resampling, channel-concat input).  Same tensor conventions as fg_edm_run_block (NHWC fp32 x1 / x2 / dout / dx1 / dx2,
 * emb and demb [B, emb_channels]).  The block's forward is recomputed first.  Parameter gradients are ACCUMULATED into the fp32
 * buffers bound with fg_edm_bind_grad (same names and shapes as the parameters; unbound = not computed); demb is accumulated as
 * well (zero it first); dx1 / dx2 are overwritten (either may be NULL). */
FG_API int fg_edm_bind_grad(fg_edm* h, const char* name, float* grad, int64_t numel);
FG_API size_t fg_edm_block_backward_workspace_bytes(const fg_edm* h, int index, int batch);
FG_API int fg_edm_run_block_backward(fg_edm* h, int index, const float* x1, int c1, const float* x2, int c2, const float* emb,
                              const float* dout, float* dx1, float* dx2, float* demb, int batch, void* workspace,
                              size_t workspace_bytes, void* stream);

/* Whole-network backward (bf16 or bf16x3 compute mode; the exact-fp32 mode has none) of EDMPrecond.forward, what autograd computes for the student / fake-score network in
 * fastgen/methods/distribution_matching/dmd2.py.  have_forward == 0: runs the kept forward itself first (-> out, as
 * fg_edm_forward_train); have_forward != 0: a fg_edm_forward_train of the same batch / workspace / inputs precedes this call and its
 * per-block stash is differentiated as it stands - nothing but the cheap conv operands silu(norm(x)) is recomputed.  dout [B,C,H,W]
 * fp32 is dL/d(out).  Gradients of all bound parameters (fg_edm_bind_grad) are ACCUMULATED.  The gradient of x_t and gradients
 * arriving at the feature taps are served by fg_edm_backward_ex below (this entry point = that one with dfeatures = dx_t = NULL). */
FG_API size_t fg_edm_backward_workspace_bytes(const fg_edm* h, int batch);
FG_API int fg_edm_backward(fg_edm* h, const float* x_t, const double* t, const double* r, const float* labels, const float* dout,
                    float* out, int have_forward, int batch, void* workspace, size_t workspace_bytes, void* stream);
/* The forward half on its own (-> out), leaving in `workspace` (sized by fg_edm_backward_workspace_bytes) what the backward
 * reads.  A following fg_edm_backward(..., have_forward = 1, same batch, same workspace, same x_t / labels) skips its own
 * forward (out may then be NULL); nothing else may write to that workspace in between. */
FG_API int fg_edm_forward_train(fg_edm* h, const float* x_t, const double* t, const double* r, const float* labels, float* out,
                         float* const* features, int batch, void* workspace, size_t workspace_bytes, void* stream);
/* fg_edm_backward with the gradient paths DMD2's GAN branch uses (dmd2.py:137-146: the frozen teacher's feature taps feed the
 * discriminator, whose loss is differentiated back to the teacher's INPUT): dfeatures[tap] (array as in fg_edm_forward_features,
 * entries nullable, NCHW fp32) joins the gradient of that encoder output; dout == NULL means the forward returned the taps early
 * and only the encoder is differentiated; dx_t (nullable, [B,C,H,W] fp32) receives dL/dx_t.  features / out of
 * fg_edm_forward_train follow fg_edm_forward_features (out == NULL: early return). */
FG_API int fg_edm_backward_ex(fg_edm* h, const float* x_t, const double* t, const double* r, const float* labels, const float* dout,
                       const float* const* dfeatures, float* out, float* dx_t, int have_forward, int batch, void* workspace,
                       size_t workspace_bytes, void* stream);

/* fg_edm_backward_ex in up to three calls, in this order, on the same arguments and workspace (the state in between lives in the
 * workspace; nothing else may write to it): FG_BWD_DECODER = [kept forward if have_forward == 0] + output head + decoder blocks,
 * FG_BWD_ENCODER = feature-tap gradients + encoder blocks + stem (+ dx_t), FG_BWD_EMBED = embedding MLP.  When a call returns, every
 * parameter gradient of its part is enqueued complete - a data-parallel wrapper can start reducing the decoder's gradients while
 * the encoder is still being differentiated (the module's autograd nodes are split this way, fastgen/utils/distributed/ddp.py:44-72).
 * parts is a mask: FG_BWD_DECODER | FG_BWD_ENCODER | FG_BWD_EMBED in one call is fg_edm_backward_ex. */
#define FG_BWD_DECODER 1
#define FG_BWD_ENCODER 2
#define FG_BWD_EMBED 4
FG_API int fg_edm_backward_part(fg_edm* h, const float* x_t, const double* t, const double* r, const float* labels, const float* dout,
                                const float* const* dfeatures, float* out, float* dx_t, int have_forward, int parts, int batch,
                                void* workspace, size_t workspace_bytes, void* stream);

/* One head of Discriminator_EDM (networks/discriminators.py:62-137) on a [B,256,res,res] NCHW fp32 feature tap, res in {8,16,32}:
 * strided 4x4 convs + GroupNorm + SiLU down to 1x1, then a 1x1 conv to one logit per image.  params: fg_disc_edm_num_params(res)
 * device pointers in the reference's module order ({conv.weight, conv.bias, gn.weight, gn.bias} per strided conv, then the 1x1
 * conv's weight and bias), fp32, reference shapes.  dlogits == NULL: forward only.  Otherwise also the backward of the same call:
 * dfeat (nullable, overwritten) and grads (nullable array / entries; same order and shapes as params; accumulated). */
FG_API int fg_disc_edm_num_params(int res);
FG_API size_t fg_disc_edm_workspace_bytes(int res, int batch);
FG_API int fg_disc_edm_run(const float* feat, int res, const float* const* params, float* logits, const float* dlogits, float* dfeat,
                    float* const* grads, int batch, void* workspace, size_t workspace_bytes, void* stream);

/* Forward-mode derivative (`torch.func.jvp(net, (x_t, t, r), tangents)` in MeanFlowModel._jvp / sCM,
 * consistency_model/mean_flow.py:240-250, sCM.py:179): out = EDMPrecond.forward(x_t, t, r), jvp = its directional derivative along
 * (vx [B,C,H,W], vt [B], vr [B]) (vt / vr nullable = 0; fp32).  bf16 or bf16x3 compute mode; workspace sized by
 * fg_edm_backward_workspace_bytes (the pass runs next to the kept forward and reuses its per-block stash). */
FG_API int fg_edm_jvp(fg_edm* h, const float* x_t, const double* t, const double* r, const float* labels, const float* vx, const float* vt,
               const float* vr, float* out, float* jvp, int batch, void* workspace, size_t workspace_bytes, void* stream);

/* The module's train()/eval() state as far as the arithmetic depends on it: `sigma_shift = None if self.training else
 * self.sigma_shift` (EDM/network.py:956).  training != 0: every following forward / backward / jvp / sampler call of this handle
 * evaluates precond_output without the shift; 0 (the state of a new handle): with cfg.sigma_shift.  Dropout is separate
 * (fg_edm_set_dropout): the reference's F.dropout also follows self.training, the module mirrors that when it sets both. */
FG_API int fg_edm_set_training(fg_edm* h, int training);

/* Augmentation labels of the training-time augmentation pipeline (EDM/network.py:495, 518-519, 903-915: condition =
 * {"aug_condition", "orig_condition"}): [B, augment_dim] fp32, added to the mapping network's input through map_augment by every
 * following forward / backward / jvp call of this handle until reset with NULL (borrowed pointer; must cover the call's batch). */
FG_API int fg_edm_set_augment(fg_edm* h, const float* augment_labels);

/* Training-mode dropout of conv1's operand in every UNetBlock (EDM/network.py:283-284; the SFT config trains with p = 0.13):
 * honoured by fg_edm_forward_train / fg_edm_backward(_ex) / fg_edm_jvp (never by the inference entry points), p = 0 turns it off.
 * The mask is Philox4x32-10(seed; element, block) - the backward regenerates it - so a forward and its backward must see the same
 * (p, seed); set p before sizing the workspace (one more tensor per block).  fg_op_dropout_mask writes the keep factors
 * (0 or 1/(1-p)) of one block's operand, flattened [B, H*W, C] (parity tests). */
FG_API int fg_edm_set_dropout(fg_edm* h, float p, uint64_t seed);
FG_API int fg_op_dropout_mask(float* out, int64_t total, float p, uint32_t block_index, uint64_t seed, void* stream);

/* ---- EDM training kernels, one op per call (bwd.hip, attn_bwd.hip): the launchers fg_edm_run_block_backward / fg_edm_backward /
 * fg_edm_jvp run, without a handle, for per-op parity tests.  Activation tensors are void* NHWC in the storage type `dtype`: 0 fp32
 * (the bf16x3 mode's storage), 1 bf16.  Every argument is checked before anything is launched; a shape the launcher cannot serve is
 * FG_EINVAL.  Dropout arguments (p, block index, seed) as fg_op_dropout_mask; p = 0: off.
 *
 * GroupNorm ops: x = the virtual concat [x1 (c1) | x2 (c2)], c1 / c2 multiples of 8, groups = min(32, C / 4); the statistics are
 * computed by the call itself (launch_gn_coeffs).  workspace: fg_op_gn_workspace_bytes(batch, c1 + c2), 16-byte aligned.
 * fg_op_gn_act: out [batch][res][res][C] = R(act(x)) * keep, act = silu(a x + b) (mode 0), a x + b (mode 1), x (mode 2: gamma, beta and
 * the workspace unused); R: rm 0 none, 1 mean of 2x2 (x at 2 res), 2 nearest 2x (x at res / 2).
 * fg_op_gn_backward: dx (+)= d(act(x))/dx applied to R^T(dact) * keep [+ add_scale * R^T(add)], x at `res`, dact (pixel pitch cd >= C)
 * and add (nullable, pitch ca) at res (rm 0), res / 2 (rm 1) or 2 res (rm 2); mode 0 / 1 as above.  dgamma / dbeta (nullable, [C]) are
 * accumulated.  dx2 == NULL: dx is [batch][res * res][C]; otherwise dx takes channels [0, c1) and dx2 [c1, C), both dense.
 * fg_op_gn_jvp: out = the tangent of act(x) along xd (dense [batch][res * res][C]) * keep; mode 0 / 1. */
FG_API size_t fg_op_gn_workspace_bytes(int batch, int c);
FG_API int fg_op_gn_act(int dtype, int mode, const void* x1, int c1, const void* x2, int c2, const float* gamma, const float* beta, float eps,
                        void* out, int batch, int res, int rm, float drop_p, uint32_t drop_block, uint64_t drop_seed, void* workspace,
                        size_t workspace_bytes, void* stream);
FG_API int fg_op_gn_backward(int dtype, int mode, const void* x1, int c1, const void* x2, int c2, const void* dact, int cd,
                             const float* gamma, const float* beta, float eps, float* dgamma, float* dbeta, const void* add, int ca,
                             float add_scale, void* dx, void* dx2, int accumulate, int batch, int res, int rm, float drop_p,
                             uint32_t drop_block, uint64_t drop_seed, void* workspace, size_t workspace_bytes, void* stream);
FG_API int fg_op_gn_jvp(int dtype, int mode, const void* x1, int c1, const void* x2, int c2, const void* xd, const float* gamma,
                        const float* beta, float eps, void* out, int batch, int res, float drop_p, uint32_t drop_block, uint64_t drop_seed,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Single-head self-attention, P = softmax(q k^T / sqrt(c)), o = P v: q, k, d_out, dq, dk, qd, kd, od [batch][t][c]; vt, dvt, vtd
 * [batch][c][t]; t in {64, 256}, c % 32 == 0.  backward: dq, dk, dvt, and (dqkv nullable) their interleave [batch][t][3 c] with channel
 * 3 ch + {0 q, 1 k, 2 v}.  jvp: od = Pd v + P vd.  workspace: fg_op_attention_backward_workspace_bytes (0: unsupported), 256-byte
 * aligned, for both. */
FG_API size_t fg_op_attention_backward_workspace_bytes(int dtype, int batch, int t, int c);
FG_API int fg_op_attention_backward(int dtype, const void* q, const void* k, const void* vt, const void* d_out, void* dq, void* dk, void* dvt,
                                    void* dqkv, int batch, int t, int c, void* workspace, size_t workspace_bytes, void* stream);
FG_API int fg_op_attention_jvp(int dtype, const void* q, const void* k, const void* vt, const void* qd, const void* kd, const void* vtd,
                               void* od, int batch, int t, int c, void* workspace, size_t workspace_bytes, void* stream);
/* out[n * out_stride + ch] = scale * sum_p t[n][p][ch] for ch < c (t has pixel pitch ct >= c; out_stride 0 = c);
 * out[ch] (and out2[ch], nullable) += sum_n in[n * in_stride + ch] (in_stride 0 = c). */
FG_API int fg_op_colsum(int dtype, const void* t, int ct, int c, float* out, int batch, int hw, float scale, int out_stride, void* stream);
FG_API int fg_op_batchsum_add(const float* in, float* out, float* out2, int batch, int c, int in_stride, void* stream);
/* Linear backward, each of dw / db / dx nullable and accumulated: dw[c][k] += scale * sum_b dy[b][ch] x[b][kk], db[ch] += sum_b dy,
 * dx[b][kk] += sum_ch dy[b][ch] w[ch][kk]; dy_stride (0 = c) is honoured by dw alone.  affine != 0: the embedding-affine kernels
 * (no db, scale 1, no stride). */
FG_API int fg_op_linear_backward(int affine, const float* dy, const float* x, const float* w, float* dw, float* db, float* dx, int batch,
                                 int c, int k, float scale, int dy_stride, void* stream);
/* Weights of the data-gradient convolution: wt[ci][co][tap] = w[co][ci][taps - 1 - tap] for ci < cin, 0 for cin <= ci < cin_pad. */
FG_API int fg_op_dgrad_weights(const float* w, float* wt, int cout, int cin, int cin_pad, int taps, void* stream);
/* The small elementwise pieces of the whole-network passes, selected by op (operands a .. e, meaning per op):
 * HEAD_GRAD out[n][p][cp] = c_out[n] dout[n][ch][p] | 0 (a dout NCHW, b c_out);  STEM_OPERAND the same with a = x, b = c_in;
 * INPUT_GRAD out[n][ch][p] = c_in[n] da[n][p][ch] (+ c_skip[n] dout) (a da with pitch ch_pad, b c_in, c c_skip, d dout nullable);
 * ADD_NCHW_TO_NHWC out[n][p][ch] += a[n][ch][p];  SILU_BWD out = a silu'(b), batch * ch elements;
 * JVP_COEF out[8][batch] from a = t, b = r (doubles, r nullable), c = vt, d = vr (nullable), f0 = sigma_data, f1 = sigma_shift,
 * flag = drop_precond;  JVP_EMBED out[batch][ch] from a = c_noise, b = r_noise, c = dc, d = dr, e = freqs, ch_pad = noise channels;
 * JVP_INPUT out = c_in vx + dc_in x (a vx, b x, c c_in, d dc_in);  JVP_OUTPUT out = c_out Fd + dc_out F + c_skip vx + dc_skip x
 * (a Fd with pitch ch_pad, b F, c x, d vx, e the JVP_COEF table). */
#define FG_TRAIN_OP_HEAD_GRAD 0
#define FG_TRAIN_OP_STEM_OPERAND 1
#define FG_TRAIN_OP_INPUT_GRAD 2
#define FG_TRAIN_OP_ADD_NCHW_TO_NHWC 3
#define FG_TRAIN_OP_SILU_BWD 4
#define FG_TRAIN_OP_JVP_COEF 5
#define FG_TRAIN_OP_JVP_EMBED 6
#define FG_TRAIN_OP_JVP_INPUT 7
#define FG_TRAIN_OP_JVP_OUTPUT 8
FG_API int fg_op_train_elementwise(int op, int dtype, const void* a, const void* b, const void* c, const void* d, const void* e, void* out,
                                   int batch, int ch, int ch_pad, int hw, double f0, double f1, int flag, void* stream);

/* ---- EDM (SongUNet) inference kernels, one op per call (conv.hip, conv_ws.hip, conv_ws3.hip, misc.hip, aux.hip, attn.hip): the
 * launchers fg_edm_forward runs, without a handle, for per-op parity tests.  dtype is a compute mode FG_DTYPE_F32 / _BF16 / _BF16X3;
 * activation tensors are void* NHWC in its storage type (bf16 in FG_DTYPE_BF16, else fp32).  Every argument is checked before anything
 * is launched: a shape, alignment (tensors, weights, ab, bias, temb 16 bytes; stats 8), null pointer or combination the launcher cannot
 * serve is FG_EINVAL with the reason in fg_last_error().
 *
 * fg_op_edm_conv_pack: OIHW fp32 weights into one of the four packings (bytes: fg_op_edm_conv_pack_bytes, 0 = no such packing):
 * GENERIC conv_fused_kernel's (any dtype, ks 1 | 3; qkv_perm: the q | k | v de-interleave of the 1x1 qkv weights), WS / X3WS the
 * wave-specialised 3x3 kernels' (bf16 / bf16x3, cout 256, cin >= 128), X3SUB the per-phase merged 2x2 weights of the sub-pixel form.
 * fg_op_edm_conv: out = (conv(R(P(a x + b))) + bias + temb[n] + resid) * scale on the virtual concat x = [src1 (c1) | src2 (c2)];
 * pro 0 none, 1 a x + b, 2 silu(a x + b); res 0 none, 1 2x2 mean (hs = 2 h), 2 nearest 2x (h = 2 hs), 3 the same as four 2x2 convs on
 * the source (wpack_ws = the X3SUB packing); outmode 0 NHWC (out [batch][h][h][cout]), 1 planes q_out, k_out [batch][h h][256] and
 * vt_out [batch][256][h h] (cout 768), 4 planes q_out, vt_out (cout 512, bf16x3, 16x16).  temb [batch][temb_stride] and resid nullable;
 * rshift 1: resid is [batch][h/2][h/2][cout] and pixel (y, x) adds its pixel (y >> 1, x >> 1).  stats (nullable) [batch][slots][cout / 4]
 * {sum, sum of squares} of the stored values per tile and channel quad.  wpack_ws NULL keeps the call on conv_fused_kernel.
 * fg_op_edm_conv_plan launches nothing and needs no GPU: the kernel launch_conv_fused will take for these arguments and the number of
 * statistics slots per image it writes, from the launcher's own predicates (FASTGEN_AMD_CONV_WS, read once per process, included). */
#define FG_EDM_PACK_GENERIC 0
#define FG_EDM_PACK_WS 1
#define FG_EDM_PACK_X3WS 2
#define FG_EDM_PACK_X3SUB 3
#define FG_EDM_CONV_GENERIC 1 /* conv_fused_kernel */
#define FG_EDM_CONV_WS 2      /* conv3_ws_kernel */
#define FG_EDM_CONV_X3WS 3    /* conv3_x3ws_kernel */
typedef struct fg_edm_conv_plan {
    int kernel;     /* FG_EDM_CONV_* */
    int stat_slots; /* statistics slots per image */
} fg_edm_conv_plan;
FG_API size_t fg_op_edm_conv_pack_bytes(int dtype, int layout, int cout, int cin, int ks);
FG_API int fg_op_edm_conv_pack(int dtype, int layout, const float* w_oihw, void* packed, int cout, int cin, int ks, int qkv_perm, void* stream);
FG_API int fg_op_edm_conv_plan(int dtype, int ks, int pro, int res, int outmode, int c1, int c2, int batch, int hs, int h, int cout,
                               int has_wpack_ws, int rshift, fg_edm_conv_plan* plan);
FG_API int fg_op_edm_conv(int dtype, int ks, int pro, int res, int outmode, const void* src1, int c1, const void* src2, int c2, int batch, int hs,
                          int h, const float* ab, const void* wpack, const void* wpack_ws, const float* bias, const float* temb, int temb_stride,
                          const void* resid, int rshift, float scale, void* out, int cout, float* stats, void* q_out, void* k_out, void* vt_out,
                          void* stream);
/* GroupNorm coefficients ab [batch][c1 + c2] {a, b} (and mr [batch][groups] {mean, rstd}, nullable) from the producers' partial
 * statistics st1 [batch][s1][c1 / 4], st2 [batch][s2][c2 / 4] (launch_gn_finalize); 16 <= c1 + c2 <= 512.
 * fg_op_edm_gn_silu_pool: out [batch][res_out][res_out][c] = mean of 2x2 of silu(a x + b), x at 2 res_out. */
FG_API int fg_op_edm_gn_finalize(const float* st1, int c1, int s1, const float* st2, int c2, int s2, const float* gamma, const float* beta,
                                 float eps, float* ab, float* mr, int batch, int hw, void* stream);
FG_API int fg_op_edm_gn_silu_pool(int dtype, const void* x, const float* ab, void* out, int batch, int res_out, int c, void* stream);
/* One head of dim 256 over t in {64, 256} tokens: out [batch][t][256] = softmax(q k^T / 16) v, q, k [batch][t][256], vt [batch][256][t].
 * merge_weights: w_out [2 c][c] = [Wk^T Wq ; Wp Wv], b_out [2 c] = [Wk^T bq ; Wp bv] from the reference's qkv_w [3 c][c] (row 3 ch + plane).
 * attention_merged (bf16x3, 256 tokens): out = (softmax(qm xn^T / 16) vm + bp + x_mid) * scale, xn = a x_mid + b; stats (nullable)
 * [batch][8][64] of out, slot = 32 tokens. */
FG_API int fg_op_edm_attention(int dtype, const void* q, const void* k, const void* vt, void* out, int batch, int t, void* stream);
FG_API int fg_op_edm_attn_merge_weights(const float* qkv_w, const float* qkv_b, const float* proj_w, float* w_out, float* b_out, int c,
                                        void* stream);
FG_API int fg_op_edm_attention_merged(const float* qm, const float* x_mid, const float* ab, const float* vmt, const float* bp, float scale,
                                      float* out, float* stats, int batch, void* stream);
/* Stem and output head.  coef [5][batch] = c_in, c_noise, c_skip, c_out, r_noise (an input here).  stem (MFMA, 128 channels out;
 * stats [batch][res res / 32][32]) and conv_in (the plain form): out NHWC = conv3x3(c_in[n] x) + bias, x NCHW fp32.  aux_head (MFMA,
 * 32x32) and aux_out (the plain form, cout <= 4): out NCHW fp32 = c_skip[n] x_t + c_out[n] (conv3x3(silu(a x + b)) + bias).  `packed`:
 * scratch for the packed weights, fg_op_edm_head_pack_bytes(FG_EDM_PACK_STEM | FG_EDM_PACK_AUX, dtype, c) bytes (0: unsupported). */
#define FG_EDM_PACK_STEM 0
#define FG_EDM_PACK_AUX 1
FG_API size_t fg_op_edm_head_pack_bytes(int which, int dtype, int c);
FG_API int fg_op_edm_stem(int dtype, const float* x, const float* coef, const float* w_oihw, void* packed, const float* bias, void* out,
                          float* stats, int batch, int res, int cin, void* stream);
FG_API int fg_op_edm_conv_in(int dtype, const float* x, const float* coef, const float* w_oihw, const float* bias, void* out, int batch, int res,
                             int cin, int cout, void* stream);
FG_API int fg_op_edm_aux_head(int dtype, const void* x, const float* ab, const float* w_oihw, void* packed, const float* bias, const float* x_t,
                              const float* coef, float* out, int batch, int c, int cout, void* stream);
FG_API int fg_op_edm_aux_out(int dtype, const void* x, const float* ab, const float* w_oihw, const float* bias, const float* x_t,
                             const float* coef, float* out, int batch, int res, int c, int cout, void* stream);

/* ---- DiT: the class-conditional diffusion transformer of fastgen/networks/DiT/network.py -------------------------
 * kwargs of DiT(input_size, patch_size, in_channels, hidden_size, depth, num_heads, mlp_ratio, num_classes, class_dropout_prob,
 * r_timestep, ...) (:233-253; configs/net.py:98-127).  Supported: token grids input_size / patch_size of 16 (256
 * tokens) and 32 (1024 tokens: the 512 x 512 models; every compute mode but FG_DTYPE_F32, and not with FASTGEN_AMD_DIT_GEMM=0 /
 * FASTGEN_AMD_DIT_GEMM3=0, which fg_dit_pack_weights / fg_dit_pack_group then refuse), hidden_size in {384, 768, 1024, 1152} with head
 * dim 64 or 72 (DiT-S/2, B/2, L/2, XL/2), mlp_hidden % 128 == 0. */
typedef struct fg_dit_config {
    int input_size;      /* 32 (latent resolution); 64 for the 512 x 512 models */
    int patch_size;      /* 2 */
    int in_channels;     /* 4 */
    int hidden_size;     /* 1152 */
    int depth;           /* 28 */
    int num_heads;       /* 16 */
    int mlp_hidden;      /* int(hidden_size * mlp_ratio) = 4608 */
    int embedding_rows;  /* num_classes + (class_dropout_prob > 0): rows of y_embedder.class_embeddings (:116-118) */
    int r_timestep;      /* 1: second time embedding r_embedder (:276-279) */
    int compute_dtype;   /* FG_DTYPE_* */
} fg_dit_config;
typedef struct fg_dit fg_dit; /* opaque */

FG_API int fg_dit_create(const fg_dit_config* cfg, fg_dit** out);
FG_API void fg_dit_destroy(fg_dit* h);
/* State-dict view: the reference's names and shapes (restated timm attribute names for the patch embedding / attention / MLP
 * layers), `pos_embed` (a persistent buffer there) included.  bind + pack: unlike the fg_edm handle (it borrows its parameters' memory until
 * the next pack) this engine copies at pack time - see fg_dit_pack_group. */
FG_API int fg_dit_num_params(const fg_dit* h);
FG_API int fg_dit_param_info(const fg_dit* h, int index, const char** name, int* ndim, int64_t shape[4]);
FG_API int fg_dit_bind_param(fg_dit* h, const char* name, const float* device_ptr, int64_t numel);
FG_API int fg_dit_pack_weights(fg_dit* h, void* stream);
/* fg_dit_pack_weights for the parameters whose names start with `prefix` and not with `exclude` (nullable) - "blocks.7.", "x_embedder.",
 * ... : the unit a sharded-data-parallel wrapper gathers at a time (DiT.fully_shard, DiT/network.py:402-420).  Packing COPIES: the block
 * linears into their GEMM layouts, every other parameter into engine-owned fp32 storage, so a bound pointer is read during
 * fg_dit_pack_group / fg_dit_pack_weights only and may be freed once that call's work on `stream` has been ordered before the free.
 * fg_dit_forward runs once every parameter has been packed since its last bind. */
FG_API int fg_dit_pack_group(fg_dit* h, const char* prefix, const char* exclude, void* stream);
FG_API size_t fg_dit_workspace_bytes(const fg_dit* h, int batch);
/* The network part of DiT.forward (:511-547): patch embedding + positional table, conditioning vector, the transformer blocks,
 * output projection, unpatchify.  x_t, out: [B,C,H,W] fp32; t, r: [B] fp32 AS THE EMBEDDERS SEE THEM (after prepare_t's rescaling,
 * :457-462, the SiT flip :503-504 and, for time_cond_type 'diff', the t - r difference :520-521: scalar host-side plumbing);
 * r NULL = no r embedding; class_ids: [B] int64 row of the class table (num_classes = the unconditional row, :493-498); an id outside
 * [0, embedding_rows) makes that sample's output NaN and the NEXT call on the handle return FG_EINVAL (the reference's nn.Embedding
 * device-asserts; the check cannot surface in the asynchronous call itself);
 * cond_out (nullable): [B, hidden_size] conditioning vector c.  Prediction-type conversion and the SiT sign stay with the caller. */
FG_API int fg_dit_forward(fg_dit* h, const float* x_t, const float* t, const float* r, const int64_t* class_ids, float* out,
                          float* cond_out, int batch, void* workspace, size_t workspace_bytes, void* stream);

/* fg_dit_forward with the block-output taps of DiT.forward (`feature_indices` / `return_features_early`, :483-484, 536-543, 563-566):
 * feature_blocks: HOST array of num_features ascending block indices; features: HOST array of as many device buffers, each
 * [B, tokens, hidden_size] fp32 = the token tensor behind that block.  out == NULL: return after the last requested block. */
FG_API int fg_dit_forward_features(fg_dit* h, const float* x_t, const float* t, const float* r, const int64_t* class_ids, float* out,
                                   float* cond_out, const int* feature_blocks, float* const* features, int num_features, int batch,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* Forward-mode derivative of fg_dit_forward (the tangent of the MeanFlow objective, fastgen/methods/consistency_model/mean_flow.py:220-252:
 * torch.func.jvp(net_wrapper, (x_t, t, r), (dxt_dt, 1, 0))).  Forward-only and stateless: no activations are kept, nothing is built for
 * a backward pass.  Served by FG_DTYPE_BF16X3 handles on a 16 x 16 token grid (every hidden size, head dims 64 and 72, r_timestep on
 * or off); any other handle has no jvp.
 * fg_dit_jvp_workspace_bytes: 0 where this handle's compute mode / token grid has no jvp. */
FG_API size_t fg_dit_jvp_workspace_bytes(const fg_dit* h, int batch);
/* out = the raw network output of fg_dit_forward(x_t, t, r, class_ids) (same arithmetic, not the same bits: the pass keeps
 * pre-activations the forward fuses away); jvp = its directional derivative along (vx [B,C,H,W], vt [B], vr [B]).  t, r, vt, vr are
 * fp32 and refer to the values AS THE EMBEDDERS SEE THEM (after scale_t / 1 - t / t - r, exactly like fg_dit_forward's t and r: the
 * caller applies the chain rule of that preparation to vt, vr).  vt / vr nullable = 0.  r / vr ignored without r_timestep; r NULL = no
 * r embedding.  FG_EINVAL before anything is launched: a null pointer, batch <= 0, a workspace that is not 256-byte aligned, out / jvp
 * overlapping an input, the workspace or each other, a handle without a jvp; FG_ENOTREADY: unpacked weights; FG_ENOMEM: workspace too
 * small.  An out-of-range class id is reported as in fg_dit_forward. */
FG_API int fg_dit_jvp(fg_dit* h, const float* x_t, const float* t, const float* r, const int64_t* class_ids, const float* vx, const float* vt,
                      const float* vr, float* out, float* jvp, int batch, void* workspace, size_t workspace_bytes, void* stream);
/* The three kernels fg_dit_jvp adds (dit_jvp.hip), handle-free, for the per-op parity tests (fp64 mirror: tests/dit_jvp_ref.py).
 * Every argument is checked before anything is launched (FG_EINVAL); pointers 16-byte aligned.
 * fg_op_dit_ln_modulate_jvp: LayerNorm (eps 1e-6, no affine) + adaLN modulation with tangent.  x, xd fp32 [ntok][d]; mod, modd
 * [ntok / tokens_per_image][mod_stride] with shift at shift_off and scale at scale_off (even numbers); y, yd: [hi | lo] bf16 planes
 * [ntok][2 d] of y = n (1 + scale) + shift and yd = nd (1 + scale) + n scaled + shiftd, n = LN(x),
 * nd = (xd - mean(xd) - n mean(n xd)) / sigma.  d in {384, 768, 1024, 1152}. */
FG_API int fg_op_dit_ln_modulate_jvp(const float* x, const float* xd, const float* mod, const float* modd, int mod_stride, int shift_off,
                                     int scale_off, void* y, void* yd, int ntok, int d, int tokens_per_image, void* stream);
/* fg_op_dit_attention (FG_DTYPE_BF16X3 layouts: hi / lo bf16 planes lo_off elements apart, 32 rows of slack behind vt / vtd) with
 * tangent: out = softmax(q k^T / sqrt(head_dim)) v, outd = (P o (Sd - delta)) v + P vd with Sd = (qd k^T + q kd^T) / sqrt(head_dim),
 * delta_i = sum_j P_ij Sd_ij; out, outd fp32 [batch][tokens][heads * head_dim].  tokens == 256, head_dim 64 or 72. */
FG_API int fg_op_dit_attention_jvp(const void* q, const void* k, const void* vt, const void* qd, const void* kd, const void* vtd, float* out,
                                   float* outd, int batch, int heads, int head_dim, int tokens, size_t lo_off, void* stream);
/* a = GELU_tanh(h), ad = GELU_tanh'(h) hd: h, hd fp32 [m][k]; a, ad [hi | lo] bf16 planes [m][2 k]; k % 4 == 0. */
FG_API int fg_op_dit_gelu_jvp(const float* h, const float* hd, void* a, void* ad, int64_t m, int k, void* stream);

/* The sampling loops around fg_dit_forward as ONE call (replayed as one hipGraph per (batch, steps, pointers) when use_graph != 0):
 *   FG_LOOP_X0        FastGenModel.generator_fn + _student_sample_loop (methods/model.py:315-420): x = noise * sigma(t_0); per step
 *                     x0 = convert(forward(x, t_i)) [flow -> x0: x - t v, fp64]; if t_{i+1} > 0: x = alpha(t_{i+1}) x0 + sigma(t_{i+1}) eps_i
 *                     ('ode': eps_i = x0_to_eps(x, x0, t_i)); returns the last x0.
 *   FG_LOOP_MEANFLOW  MeanFlowModel._student_sample_loop (consistency_model/mean_flow.py:336-381), as fg_sampler_run's.
 *   FG_LOOP_EULER     DiT._sample_flow (DiT/network.py:605-651): x += fp32(t_{i+1} - t_i) * v, with neg_class_ids != NULL
 *                     v = v_uncond + guidance_scale * (v_cond - v_uncond) from ONE forward of the doubled batch [x | x], [neg | cond].
 * The time conditioning that DiT.forward derives on the host (prepare_t's rescaling :457-462, the SiT flip :503-504 and sign :555-558,
 * the 'diff' form of r :520-521) is described by fg_dit_sampler_config and evaluated on the device from the resident t_list.
 * noise, out: [B,C,H,W] fp32; class_ids / neg_class_ids: [B] int64; t_list: HOST array of steps+1 doubles ending in 0; eps as for
 * fg_sampler_run.  Bit-identical to the same loop run step by step through fg_dit_forward and the fg_op_* elementwise kernels. */
typedef struct fg_dit_sampler_config {
    double t_scale;          /* the embedder sees fp32(t_scale * t): noise_scheduler.num_steps (1000) with scale_t on the RF schedule, else 1 */
    double guidance_scale;   /* FG_LOOP_EULER with neg_class_ids */
    int use_sit_convention;  /* t_e = 1 - t_e, flow output negated */
    int time_cond_diff;      /* time_cond_type == "diff": r_e = t_e - r_e */
    int net_pred_flow;       /* net_pred_type == "flow" (1) or "x0" (0) */
    int schedule;            /* FG_SCHEDULE_* of net.noise_scheduler */
} fg_dit_sampler_config;
FG_API size_t fg_dit_sampler_workspace_bytes(const fg_dit* h, int batch, int guided);
FG_API int fg_dit_sampler_run(fg_dit* h, const fg_dit_sampler_config* cfg, const float* noise, const int64_t* class_ids,
                              const int64_t* neg_class_ids, const double* t_list, int steps, int sample_type, int loop_kind, const float* eps,
                              uint64_t seed, float* out, int batch, void* workspace, size_t workspace_bytes, int use_graph, void* stream);

/* ---- Causal video DiT (SURVEY 8(f)3 and the CausVid row of 8(a); reference fastgen/networks/Wan/network_causal.py `CausalWan`, driven
 * chunk by chunk by `CausVidModel._student_sample_loop`, fastgen/methods/distribution_matching/causvid.py:87-185) --------------
 * The arithmetic of this network is diffusers' WanTransformer3DModel (un-vendored, diffusers==0.35.1): the HIP path follows the
 * restatement in oracle/wan_ref.py - PARITY UNPINNED.  bf16 token tensors and GEMM operands with fp32 accumulation,
 * fp32 norms / softmax / modulation: the reference runs this network in bf16 (configs/experiments/WanT2V/config_sf.py:19).
 * fg_wan_config = the fields of the transformer's config the path reads.  Supported: head_dim 128, inner dim (heads x 128) in
 * {256, 384, 1536 (1.3B), 2048, 3072 (5B), 5120 (14B)}, patch (1,2,2), ffn_dim / text_dim % 64 == 0, freq_dim 256, cross_attn_norm.
 * compute_dtype FG_DTYPE_FP8: the six linears of a block that read the video tokens - attn1 to_q | to_k | to_v (one fused GEMM),
 * attn1.to_out.0, attn2.to_q, attn2.to_out.0, ffn.net.0.proj, ffn.net.2 - run on e4m3fn operands (FG_DTYPE_FP8 above: weights
 * re-quantised per output channel on every pack, the LayerNorm-modulate outputs, the two attention outputs and the GELU hidden
 * quantised per token); the text side (text_embedder, attn2.to_k / to_v: once per text in fg_wan_set_text), time embedder, patch
 * embedding, proj_out, attention, RMSNorm + RoPE and the caches are the bf16 mode's.  ffn_dim % 128 == 0 then.  Through every entry
 * point below, the two samplers included; fg_wan_workspace_bytes grows by the quantised operands (m x (inner dim + ffn_dim + 8) bytes). */
typedef struct fg_wan_config {
    int num_heads;         /* 12 */
    int head_dim;          /* 128 */
    int in_channels;       /* 16 */
    int out_channels;      /* 16 */
    int text_dim;          /* 4096 */
    int freq_dim;          /* 256 */
    int ffn_dim;           /* 8960 */
    int num_layers;        /* 30 */
    int rope_max_seq_len;  /* 1024 */
    int chunk_size;        /* CausalFastGenNetwork.chunk_size, 3 (frames per autoregressive chunk; the sampler's business) */
    int total_num_frames;  /* 21: capacity of the self-attention KV caches, in frames */
    float eps;             /* 1e-6 */
    int compute_dtype;     /* 0 (unset) or FG_DTYPE_BF16: bf16 linears; FG_DTYPE_FP8; anything else: FG_EINVAL */
} fg_wan_config;
typedef struct fg_wan fg_wan; /* opaque */

FG_API int fg_wan_create(const fg_wan_config* cfg, fg_wan** out);
FG_API void fg_wan_destroy(fg_wan* h);
/* State-dict view: `transformer.` + diffusers' parameter names (the reference's CausalWan.state_dict()); shapes up to 5-d (the
 * Conv3d patch embedding); bind / pack as for fg_edm. */
FG_API int fg_wan_num_params(const fg_wan* h);
FG_API int fg_wan_param_info(const fg_wan* h, int index, const char** name, int* ndim, int64_t shape[5]);
FG_API int fg_wan_bind_param(fg_wan* h, const char* name, const float* device_ptr, int64_t numel);
FG_API int fg_wan_pack_weights(fg_wan* h, void* stream);
/* As fg_dit_pack_group: "transformer.blocks.7." packs one block, prefix "transformer." with exclude "transformer.blocks." the rest
 * (the grouping of Wan.fully_shard, Wan/network.py:761-782).  Bound pointers are read at pack time only. */
FG_API int fg_wan_pack_group(fg_wan* h, const char* prefix, const char* exclude, void* stream);
/* Workspace for one forward over a chunk of `frames` latent frames of height x width (also enough for fg_wan_set_text). */
FG_API size_t fg_wan_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width);
/* `CausalWan.clear_caches` (:1030-1054): zero the self-attention caches, forget the text (cross-attention) caches - of both cache tags. */
FG_API int fg_wan_clear_caches(fg_wan* h, void* stream);
/* The reference's `cache_tag` (:331-412): the handle keeps one cache set per tag - the per-block self-attention K / V caches, the
 * per-block cross-attention (text) caches, and their bookkeeping (batch, capacity, stored rows, text batch and length).  tag 0 = "pos"
 * (selected at creation), 1 = "neg"; anything else: FG_EINVAL.  Host-side only.  After a select, fg_wan_set_text, fg_wan_forward,
 * fg_wan_forward_features and fg_wan_sampler_run act on the selected set (fg_wan_forward_block_causal touches no cache); the overwrite
 * check of fg_wan_forward is per tag.  fg_wan_clear_caches clears both sets and packing invalidates both text caches.  A set is
 * allocated when it is first used: a handle that never selects tag 1 holds one set, as before; using it costs a second set of memory.
 * A graph captured by a sampler loop under one tag is not replayed under the other (its key holds the set's pointers). */
FG_API int fg_wan_select_cache_tag(fg_wan* h, int tag);
/* The text condition: text [B, text_len, text_dim] fp32 (the text encoder's output).  Runs condition_embedder.text_embedder and
 * every block's attn2 k / v projections (+ norm_k) once: the reference's static cross-attention cache (:331-360).  The caches are
 * rewritten in place while batch x text_len stays the same (the sampler loops' cached graphs name them); a change of that size
 * reallocates them and drops those graphs. */
FG_API int fg_wan_set_text(fg_wan* h, const float* text, int batch, int text_len, void* workspace, size_t workspace_bytes, void* stream);
/* One network call of the autoregressive sampler: `CausalWan.forward(x_t, t, cache_tag="pos", cur_start_frame, store_kv, is_ar=True)`
 * up to the raw network output (:1077-1160; the flow -> x0 conversion stays with the caller).  x_t, out: [B, C, frames, H, W] fp32;
 * t_frames: [B * frames] fp32 AS THE EMBEDDER SEES THEM (rescale_t: 1000 t, `_compute_timestep_inputs` :1063-1075).  The chunk's
 * keys / values are written to cache rows [cur_start_frame * frame_seqlen, +frames * frame_seqlen) in every call and attention runs
 * over rows [0, that end): with store_kv = 0 the rows are rewritten by the chunk's later store_kv = 1 call, as in the reference's
 * loop (causvid.py:150-172), where only that call moves the cache length.  Restriction: a store_kv = 0 call whose rows were filled by
 * an earlier store_kv = 1 call (re-evaluating a stored chunk; the reference leaves its cache untouched there) returns FG_EINVAL. */
FG_API int fg_wan_forward(fg_wan* h, const float* x_t, const float* t_frames, float* out, int batch, int frames, int height, int width,
                          int cur_start_frame, int store_kv, void* workspace, size_t workspace_bytes, void* stream);
/* The teacher- / diffusion-forcing call over ALL frames: `CausalWan.forward(x_t, t, is_ar=False)` with frames == total_num_frames, where the
 * reference attends through the block-wise causal mask of `_prepare_blockwise_causal_attn_mask` (network_causal.py:131-196, 673-680):
 * a query sees the keys up to the end of its own chunk of chunk_size frames (the first chunk also holds frames % chunk_size).
 * t_frames [B * frames] may differ per frame (diffusion forcing).  RoPE starts at frame 0; the self-attention caches are neither
 * read nor written.  fg_wan_workspace_bytes(batch, total_num_frames, ...) covers this call's extra K / V buffers. */
FG_API int fg_wan_forward_block_causal(fg_wan* h, const float* x_t, const float* t_frames, float* out, int batch, int frames, int height,
                                       int width, void* workspace, size_t workspace_bytes, void* stream);

/* Exposed for the parity tests (tests/test_gpu_wan_blocks.py): fg_wan_forward (block_causal == 0) or fg_wan_forward_block_causal
 * (block_causal != 0; cur_start_frame and store_kv must be 0) with taps inside the blocks.  tap_blocks: HOST array of num_taps
 * ascending block indices; taps: HOST array of as many structs of nullable fp32 device buffers [B, frames * frame_seqlen, inner dim],
 * each the exact widening of the bf16 buffer the next kernel consumes.  tokens_out (nullable): [B, L, D] the patch embedding;
 * temb_out (nullable): [B * frames, D] the fp32 time embedding (a copy).  The copies run on `stream` behind the kernel that wrote the
 * buffer; `out` and the caches are what the untapped call leaves. */
typedef struct fg_wan_block_taps {
    float* attn1;    /* self-attention output before to_out */
    float* x_attn1;  /* token stream after the gated self-attention residual */
    float* attn2;    /* cross-attention output before to_out */
    float* x_attn2;  /* token stream after the cross-attention residual */
    float* x_ffn;    /* token stream after the feed-forward: the block's output */
} fg_wan_block_taps;
FG_API int fg_wan_forward_features(fg_wan* h, const float* x_t, const float* t_frames, float* out, int batch, int frames, int height, int width,
                                   int cur_start_frame, int store_kv, int block_causal, const int* tap_blocks, const fg_wan_block_taps* taps,
                                   int num_taps, float* tokens_out, float* temb_out, void* workspace, size_t workspace_bytes, void* stream);

/* The chunk-by-chunk student loop of the causal video DiT as ONE call: `CausVidModel._student_sample_loop` (causvid.py:87-185), the
 * segment loop of `generator_fn_extrapolation` (:283-345, prefill_frames > 0) and the no-grad form of
 * `SelfForcingModel.rollout_with_gradient` (self_forcing.py:92-241, exit_steps != NULL).  x: [B, C, frames, H, W] fp32 latents (already
 * scaled by sigma(t_0) where the caller's generator_fn does that), overwritten in place with the generated frames.  Chunks: chunk_size
 * frames each, the remainder of frames joins the FIRST chunk.  Per chunk: for i in 0 .. last (last = steps - 1, or exit_steps[chunk]):
 * x0 = convert(fg_wan_forward(x_chunk, t_i, cur_start_frame, store_kv = 0)); unless i == last or t_{i+1} == 0 re-noise to t_{i+1} ('sde':
 * fresh noise, 'ode': the noise implied by (x_chunk, x0)); then the cache-fill call fg_wan_forward(x0 [re-noised to context_noise],
 * t = 0 [context_noise], store_kv = 1).  Chunks inside [0, prefill_frames) only run the cache-fill call at t = 0 on x as given.
 * The self-attention caches are emptied first and cleared (zeroed, text forgotten) at the end, as the reference's loop does: call
 * fg_wan_set_text before every run.  eps (nullable): steps - 1 (+ 1 if context_noise > 0) noise videos [B, C, frames, H, W] to inject,
 * indexed by re-noising step (last: the cache call's); NULL: Philox4x32-10 from (seed; chunk, step).  use_graph != 0: one hipGraph per
 * chunk (start frame, frame count and key length are baked in), replayed while shapes and pointers stay the same.  Bit-identical to
 * the same sequence of fg_wan_forward + fg_op_* calls. */
typedef struct fg_wan_sampler_config {
    double t_scale;        /* the embedder sees fp32(t_scale * t): noise_scheduler.num_steps (1000) on the RF schedule */
    double context_noise;  /* 0: the cache-fill call sees the clean chunk at t = 0 */
    int net_pred_flow;     /* net_pred_type == "flow" (1) or "x0" (0) */
    int schedule;          /* FG_SCHEDULE_* */
    int prefill_frames;    /* frames at the head of x that only fill the caches (multiple of chunk_size; frames then too) */
} fg_wan_sampler_config;
FG_API size_t fg_wan_sampler_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width);
FG_API int fg_wan_sampler_run(fg_wan* h, const fg_wan_sampler_config* cfg, float* x, const double* t_list, int steps, int sample_type,
                              const int* exit_steps, const float* eps, uint64_t seed, int batch, int frames, int height, int width,
                              void* workspace, size_t workspace_bytes, int use_graph, void* stream);

/* The autoregressive teacher sampler with classifier-free guidance as ONE call: `CausalWan.sample` (network_causal.py:1186-1295) with
 * the scheduler's step restated as a linear multistep update (fastgen_amd/networks/Wan/solvers.py builds the table; PARITY UNPINNED:
 * the reference steps diffusers' UniPCMultistepScheduler).  x: [B, C, frames, H, W] fp32, the noise, overwritten in place with the
 * sample.  Chunks as in fg_wan_sampler_run.  Per chunk, for i in 0 .. steps - 1: ONE fg_wan_forward of the stacked batch 2 B
 * ([x_chunk; x_chunk] against the text [cond; neg_cond], t = t_list[i], cur_start_frame, store_kv = 0), then one elementwise pass
 * (fg_op_guided_multistep) with table row i; then the chunk goes back into x and the cache-fill call runs on the stacked batch
 * (store_kv = 1) at t = 0, or at context_noise on the chunk re-noised with eps ([B, C, frames, H, W], one noise video; NULL:
 * Philox4x32-10 from (seed; chunk)).  guidance == 0: the same loop unstacked at batch B (the table's g is not read).  The caller sets
 * the text for the batch the loop runs at (2 B: [cond; neg_cond]) with fg_wan_set_text before every run; the loop uses the tag-0 cache
 * set (FG_EINVAL while tag 1 is selected), which therefore holds 2 B rows, empties it first and clears both sets at the end.
 * t_list: HOST array of `steps` timesteps in [0, 1] as the schedule counts them (the embedder sees fp32(t_scale * t)); table: HOST
 * array [steps][8] = {s, g, c0, c1, c2, p0, p1, p2} per step.  steps: 1 .. 4096 (the 64-step limit of the student loops does not
 * apply).  use_graph != 0: one hipGraph per chunk keyed by shapes, pointers and the step count; timesteps, table (with the guidance
 * scale) and seed live in device memory, so a replay with other values re-captures nothing.  Bit-identical to the same sequence of
 * fg_wan_forward calls at batch 2 B and fg_op_guided_multistep / fg_op_forward_process. */
typedef struct fg_wan_guided_sampler_config {
    double t_scale;        /* the embedder sees fp32(t_scale * t): noise_scheduler.num_steps (1000) on the RF schedule */
    double context_noise;  /* 0: the cache-fill call sees the clean chunk at t = 0 (RF schedule: x = (1 - c) x0 + c eps otherwise) */
    int guidance;          /* 1: stacked batch 2 B, v = v_u + g (v_c - v_u); 0: batch B */
} fg_wan_guided_sampler_config;
FG_API size_t fg_wan_guided_sampler_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width, int steps, int guidance);
FG_API int fg_wan_guided_sampler_run(fg_wan* h, const fg_wan_guided_sampler_config* cfg, float* x, const double* t_list, const double* table,
                                     int steps, const float* eps, uint64_t seed, int batch, int frames, int height, int width,
                                     void* workspace, size_t workspace_bytes, int use_graph, void* stream);
/* ---- Bidirectional video DiT (reference fastgen/networks/Wan/network.py `Wan`: the network of the DMD2 / f-distill / LADD / MeanFlow
 * WanT2V students and the teacher of all of them) on the same handle: every frame attends to every frame, no self-attention cache.
 * PARITY UNPINNED like the rest of fg_wan_*.
 * fg_wan_create_ex(cfg, NULL or an all-zero ext, ...) is fg_wan_create: the same parameter table in the same order.  r_timestep = 1
 * adds the second time embedder `r_embedder` (`init_embedder`, Wan/network.py:799-834: a deep copy of condition_embedder without its
 * text_embedder, attached after logvar_linear), six parameters behind `transformer.logvar_linear.*`:
 * transformer.r_embedder.time_embedder.linear_1.{weight,bias}, ...linear_2.{weight,bias}, transformer.r_embedder.time_proj.{weight,bias}.
 * These names and their order are read from the reference's code, not recorded from a run of it (diffusers is un-vendored). */
typedef struct fg_wan_ext_config {
    int r_timestep;      /* 1: the handle has the r_embedder */
    int time_cond_diff;  /* time_cond_type: 1 = "diff" (the r_embedder sees t - r), 0 = "abs" (r) */
} fg_wan_ext_config;
FG_API int fg_wan_create_ex(const fg_wan_config* cfg, const fg_wan_ext_config* ext, fg_wan** out);
/* `Wan.forward` up to the raw network output: all `frames` frames under full self-attention - fg_wan_forward_block_causal's path with one
 * chunk, ONE attention launch per block over this call's own K / V (the same launches as that call when chunk_size >= frames ==
 * total_num_frames).  No self-attention cache is allocated, read or written, and the caches' bookkeeping and the chunk graphs stay as
 * they are.  frames <= rope_max_seq_len (not total_num_frames).  t_frames [B * frames] as for fg_wan_forward.  r_frames (nullable)
 * [B * frames], in the embedder's units too: the r_embedder runs on fp32(t_frames - r_frames) when time_cond_diff, else on r_frames;
 * its embedding is added to temb and its projection to timestep_proj (`classify_forward_prepare`, Wan/network.py:330-351, the
 * `encoder_depth is None` branch).  r_frames on a handle without the r_embedder: FG_EINVAL; NULL on a handle with it: no r term.
 * skip_layers (nullable): HOST array of num_skip ascending block indices the call passes over (`classify_forward_block_forward`,
 * :408); out of range or unsorted: FG_EINVAL.  The text is the selected tag's (fg_wan_set_text).  Workspace:
 * fg_wan_full_workspace_bytes (also enough for fg_wan_set_text). */
FG_API size_t fg_wan_full_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width);
FG_API int fg_wan_forward_full(fg_wan* h, const float* x_t, const float* t_frames, const float* r_frames, float* out, int batch, int frames,
                               int height, int width, const int* skip_layers, int num_skip, void* workspace, size_t workspace_bytes, void* stream);
/* Exposed for the parity tests (tests/test_gpu_wan_full_blocks.py): fg_wan_forward_full with the taps of fg_wan_forward_features -
 * the same forward, the same launches, fp32 copies behind the kernels that wrote the buffers; `out` is what the untapped call leaves.
 * tap_blocks / taps / num_taps / tokens_out as there.  temb_out (nullable) [B * frames, D]: temb with the r_embedder's embedding added
 * (when r_frames is given).  tproj_out (nullable) [B * frames, 6 D]: timestep_proj with the r_embedder's projection added - the rows
 * every block's modulation is formed from.  A block that is both tapped and in skip_layers: FG_EINVAL (it runs nothing). */
FG_API int fg_wan_forward_full_features(fg_wan* h, const float* x_t, const float* t_frames, const float* r_frames, float* out, int batch,
                                        int frames, int height, int width, const int* skip_layers, int num_skip, const int* tap_blocks,
                                        const fg_wan_block_taps* taps, int num_taps, float* tokens_out, float* temb_out, float* tproj_out,
                                        void* workspace, size_t workspace_bytes, void* stream);
/* Forward-mode derivative of fg_wan_forward_full (Wan.jvp; MeanFlow's tangent): out = net(x_t, t, r) and jvp = d net . (v_x, vt, vr),
 * both [B, C, frames, H, W] fp32, from one schedule that carries a bf16 tangent stream beside the bf16 primal stream (engine_wan_jvp.inc,
 * kernels wan_jvp.hip).  t_frames, r_frames (nullable, needs the r_embedder), vt_frames, vr_frames (nullable = 0): one fp32 row entry per
 * (sample, frame), as fg_wan_forward_full takes them; under time_cond_diff the engine forms t - r and vt - vr itself.  The text is
 * fg_wan_set_text's.  `out` is fg_wan_forward_full's result up to bf16 rounding (the GELU runs on the stored bf16 pre-activation and
 * the attention kernel is the jvp's own), not to the bit.  Stateless and forward-only.  FG_EINVAL with a message, and a workspace
 * query of 0: an fp8, image-to-video (i2v / ti2v) or VACE handle; FG_EINVAL: skip_layers (non-null or num_skip != 0 - the arguments
 * exist so that a caller's skip list is refused instead of ignored), out aliasing x_t / v_x, jvp aliasing any argument, vr_frames
 * without r_frames.  FG_ENOMEM: a workspace smaller than fg_wan_jvp_workspace_bytes. */
FG_API size_t fg_wan_jvp_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width);
FG_API int fg_wan_jvp(fg_wan* h, const float* x_t, const float* t_frames, const float* r_frames, const float* v_x, const float* vt_frames,
                      const float* vr_frames, float* out, float* jvp, int batch, int frames, int height, int width, const int* skip_layers,
                      int num_skip, void* workspace, size_t workspace_bytes, void* stream);
/* Exposed for the per-op tests (tests/test_gpu_wan_jvp_ops.py) and timings: the kernels of wan_jvp.hip on their own; bf16 token tensors.
 * fg_op_wan_attention_jvp: fg_op_attention_ex's operands (head dim 128) with tangents - qd as q, kd / vd as k / v, outd as out; qd,
 * kd, vd nullable (= 0); nothing is read past key lkv - 1.  ldq, ldk, q_bs, kv_bs % 8 and 16-byte aligned q / qd / k / v / kd / vd; ldo,
 * o_bs % 4 and 8-byte aligned out / outd (FG_EINVAL otherwise).
 * fg_op_wan_modulate_jvp: y = LN(x) (1 + s) + b and its tangent; mod / modd fp32 rows of mod_stride floats (row = token /
 * tokens_per_row) with shift at shift_off and scale at scale_off; modd nullable (a constant affine).  d: 256, 384, 1536, 2048, 3072, 5120.
 * fg_op_wan_rms_rope_jvp: RMSNorm over d times w, then the pair rotation cs [l][64] {cos, sin} (nullable: none), rows [rows][ld_src] ->
 * [rows][d], token = row % l.
 * fg_op_wan_gelu_jvp: a = gelu_tanh(h), ad = gelu_tanh'(h) hd over n values (n % 4 == 0; a / ad may be h / hd).
 * fg_op_wan_final_jvp: fg_op_wan_final's wave-per-token head with tangent (modd laid out as mod: [B * frames][2][d]). */
FG_API int fg_op_wan_attention_jvp(const void* q, const void* qd, int ldq, int64_t q_bs, const void* k, const void* v, const void* kd,
                                   const void* vd, int ldk, int64_t kv_bs, void* out, void* outd, int ldo, int64_t o_bs, int batch, int heads,
                                   int lq, int lkv, void* stream);
FG_API int fg_op_wan_modulate_jvp(const void* x, const void* xd, const float* mod, const float* modd, int mod_stride, int shift_off, int scale_off,
                                  void* y, void* yd, int ntok, int d, int tokens_per_row, float eps, void* stream);
FG_API int fg_op_wan_rms_rope_jvp(const void* src, const void* srcd, int ld_src, const float* w, float eps, const float* cs, void* dst, void* dstd,
                                  int rows, int l, int d, void* stream);
FG_API int fg_op_wan_gelu_jvp(const void* h, const void* hd, void* a, void* ad, int64_t n, void* stream);
FG_API int fg_op_wan_final_jvp(const void* tokens, const void* tokens_d, const float* mod, const float* modd, const float* w, const float* bias,
                               float* out, float* outd, int batch, int channels, int frames, int gh, int gw, int d, float eps, void* stream);
/* The few-step student loops over the whole video as ONE call and one hipGraph, as fg_dit_sampler_run: loop_kind FG_LOOP_X0
 * (`FastGenModel._student_sample_loop`, methods/model.py:315-372) or FG_LOOP_MEANFLOW (`MeanFlowModel._student_sample_loop`,
 * consistency_model/mean_flow.py:336-381: r = 0 for 'sde', t_{i+1} for 'ode'; needs the r_embedder and net_pred_flow, else FG_EINVAL).
 * noise, out: [B, C, frames, H, W] fp32; latents = noise * sigma(t_0); every frame's embedder row is fp32(t_scale * t_i).  eps
 * (nullable): steps - 1 noise videos to inject; NULL: Philox4x32-10 from (seed; step).  cfg: context_noise and prefill_frames must be 0
 * (FG_EINVAL).  The graph's key holds the shapes, every buffer address, the text's length and k / v buffer, the compute mode and
 * time_cond_diff.  Bit-identical to the same sequence of fg_wan_forward_full + fg_op_* calls. */
FG_API size_t fg_wan_full_sampler_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width);
FG_API int fg_wan_full_sampler_run(fg_wan* h, const fg_wan_sampler_config* cfg, const float* noise, const double* t_list, int steps,
                                   int sample_type, int loop_kind, const float* eps, uint64_t seed, float* out, int batch, int frames,
                                   int height, int width, void* workspace, size_t workspace_bytes, int use_graph, void* stream);
/* The teacher's `Wan.sample` (Wan/network.py:919-988) as ONE call and one hipGraph for the video: fg_wan_guided_sampler_run without
 * chunks, caches, the cache-fill call and its noise (cfg->context_noise must be 0).  x: the latents (noise * sigma(t_0), the caller's
 * business), overwritten with the sample.  Per step: one fg_wan_forward_full on the stacked batch [x; x] against [cond; neg_cond]
 * (guidance == 0: batch B), then fg_op_guided_multistep with table row i.  t_list, table, steps as there; they go up through the same
 * pinned host copy.  The caller sets the text for the batch the loop runs at before the run; it is still set afterwards. */
FG_API size_t fg_wan_full_guided_sampler_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width, int steps, int guidance);
FG_API int fg_wan_full_guided_sampler_run(fg_wan* h, const fg_wan_guided_sampler_config* cfg, float* x, const double* t_list,
                                          const double* table, int steps, int batch, int frames, int height, int width, void* workspace,
                                          size_t workspace_bytes, int use_graph, void* stream);
/* Image-to-video on the bidirectional network (reference fastgen/networks/WanI2V/network.py `WanI2V`, the Wan2.1-I2V convention:
 * concat_mask = True, use_image_encoder = True).  PARITY UNPINNED like the rest of fg_wan_*.  The patch embedding reads the virtual
 * cfg->in_channels = 2 latent_channels + 4 channel tensor [x_t | mask | first_frame_cond] (mask: ones on latent frame 0, on all four
 * channels), cfg->out_channels == latent_channels, and every cross-attention adds a second, separately normalised softmax over the
 * embedded CLIP image tokens.  Parameter table: fg_wan_create_ex's with, when image_dim > 0, the eight
 * `condition_embedder.image_embedder.{norm1.weight, norm1.bias, ff.net.0.proj.weight, ff.net.0.proj.bias, ff.net.2.weight,
 * ff.net.2.bias, norm2.weight, norm2.bias}` behind `condition_embedder.text_embedder.linear_2.bias` and, in every block, the five
 * `attn2.{add_k_proj.weight, add_k_proj.bias, add_v_proj.weight, add_v_proj.bias, norm_added_k.weight}` behind `attn2.norm_k.weight`
 * (unpinned: read from the key map at Wan/network.py:1029-1049 and diffusers' module order, not recorded from a run); image_dim == 0:
 * exactly fg_wan_create_ex's table.  FG_EINVAL (the message names the field): mask_channels != 4, in_channels != 2 latent_channels +
 * mask_channels, out_channels != latent_channels, image_dim < 0 or not a multiple of 64.
 * On such a handle fg_wan_forward_full, fg_wan_forward_full_features, fg_wan_full_sampler_run and fg_wan_full_guided_sampler_run
 * take x_t / noise / x with latent_channels channels and need the condition set for the batch and (frames, height, width) of the
 * call (FG_ENOTREADY otherwise; the guided loop runs at 2 B: set text and condition for [cond; neg_cond]); the chunked and causal
 * entry points (fg_wan_forward, fg_wan_forward_block_causal, fg_wan_forward_features in those modes, fg_wan_sampler_run,
 * fg_wan_guided_sampler_run) return FG_EINVAL "not implemented for an image-to-video handle".  The Wan2.2-TI2V convention
 * (concat_mask = False, expanded timesteps) is fg_wan_create_ti2v below.  Not implemented: the image embedder's pos_embed (FLF2V). */
typedef struct fg_wan_i2v_config {
    int latent_channels;   /* 16: channels of x_t and of first_frame_cond */
    int mask_channels;     /* 4 (scale_factor_temporal): anything else FG_EINVAL */
    int image_dim;         /* 1280 (CLIP); 0: no image branch, no image parameters; else % 64 == 0 */
} fg_wan_i2v_config;
FG_API int fg_wan_create_i2v(const fg_wan_config* cfg, const fg_wan_ext_config* ext /* nullable */, const fg_wan_i2v_config* i2v, fg_wan** out);
/* The image-to-video condition, the counterpart of fg_wan_set_text: first_frame_cond [B, latent_channels, F, H, W] is copied into a
 * buffer of the handle; image [B, image_len, image_dim] (nullable; image_len 1 .. 1024, 257 for CLIP ViT-H) goes through the image
 * embedder (fp32 LayerNorm eps 1e-5 - Linear - erf GELU - Linear - fp32 LayerNorm eps 1e-5) and, per block, k_img =
 * norm_added_k(add_k_proj(tokens)) (RMSNorm over the inner dimension, like norm_k) and v_img = add_v_proj(tokens) into a bf16 cache
 * of whole 32-key tiles per sample, zero-filled.  bf16 operands in every compute mode.  image == NULL, image_len == 0 or a handle
 * with image_dim == 0: no image context (the reference's empty image context, network_causal.py:297-302) - the blocks then run the
 * text attention alone.  The buffers are rewritten in place while the shapes stay (a captured loop stays valid across new contents)
 * and reallocated otherwise.  Packing weights invalidates the condition; FG_ENOTREADY before packing.  The workspace (256-byte
 * aligned, fg_wan_i2v_cond_workspace_bytes; 0 bytes and NULL without image tokens) is scratch of this call only. */
FG_API size_t fg_wan_i2v_cond_workspace_bytes(const fg_wan* h, int batch, int image_len);
FG_API int fg_wan_set_i2v_cond(fg_wan* h, const float* first_frame_cond, const float* image, int batch, int frames, int height, int width,
                               int image_len, void* workspace, size_t workspace_bytes, void* stream);
/* Exposed for the parity tests: fp32 copies of the condition's embedded image tokens [B, image_len, D] and of block `block`'s k_img /
 * v_img [B, image_len, D] each (all nullable).  FG_ENOTREADY without an image context.  Synchronises the stream. */
FG_API int fg_wan_i2v_cond_read(fg_wan* h, int block, float* img_tokens, float* k_img, float* v_img, void* stream);
/* Wan2.2 TI2V-5B's image-to-video convention on the bidirectional network (reference fastgen/networks/WanI2V/network.py `WanI2V` with
 * concat_mask = False, use_image_encoder = False, expand_timesteps = True).  PARITY UNPINNED like the rest of fg_wan_*.  Parameter
 * table: exactly fg_wan_create_ex's (no image keys).  FG_EINVAL unless cfg->in_channels == cfg->out_channels == latent_channels.
 * The condition is frame 0 of the first-frame latents (fg_wan_set_first_frame).  On such a handle fg_wan_forward_full,
 * fg_wan_forward_full_features, fg_wan_full_sampler_run (FG_LOOP_X0) and fg_wan_full_guided_sampler_run
 *   - read frame 0's tokens from the condition instead of x_t (`_replace_first_frame`; the replaced latents are never formed),
 *   - zero the t and r embedder rows of frame 0 (the expanded per-token timesteps `mask * t` are constant within a latent frame, so
 *     they are the per-frame rows with frame 0's at zero),
 *   - write the condition into frame 0 of their result: of the network output (forward: a caller that converts the prediction type
 *     writes the condition's frame 0 again behind its conversion, as the reference does), of every x0 prediction of the x0 loop and of
 *     the latents after every solver step of the guided loop.
 * FG_ENOTREADY without a condition for the call's batch and size (the guided loop runs at 2 B: [cond; neg_cond]).  FG_EINVAL: the
 * chunked and causal entry points, and FG_LOOP_MEANFLOW (there the reference writes latents into a velocity, which a fused loop does
 * not reproduce). */
typedef struct fg_wan_ti2v_config {
    int latent_channels;   /* 48: channels of x_t, of the result and of the first-frame condition */
} fg_wan_ti2v_config;
FG_API int fg_wan_create_ti2v(const fg_wan_config* cfg, const fg_wan_ext_config* ext /* nullable */, const fg_wan_ti2v_config* ti2v, fg_wan** out);
/* first_frame [batch, latent_channels, 1, height, width] fp32 (device) is copied into a buffer of the handle, rewritten in place while
 * the shape stays (a captured loop replays on the new contents) and reallocated otherwise.  FG_EINVAL on any other handle. */
FG_API int fg_wan_set_first_frame(fg_wan* h, const float* first_frame, int batch, int height, int width, void* stream);
/* Exposed for the tests: the handle's copy into out [batch, latent_channels, 1, height, width].  FG_ENOTREADY before a condition is set. */
FG_API int fg_wan_first_frame_read(fg_wan* h, float* out, void* stream);
/* VACE: video-to-video control on the bidirectional network (reference fastgen/networks/VaceWan/network.py `VACEWan`,
 * vace_classify_forward_*; the block body is diffusers' WanVACETransformerBlock).  PARITY UNPINNED like the rest of fg_wan_*; in
 * addition the VACE keys and their order are read from diffusers' module order, not recorded from a run.  A second stack of
 * num_vace_layers "VACE blocks" runs on a control stream c and adds scaled hints into the main token stream:
 *   x0 = patch_embedding(x_t);  ctx = vace_patch_embedding(vid_context) flattened to tokens and THEN zero-padded to x0's token count
 *   (a context may have fewer frames than the video);  c = proj_in(ctx) + x0 (a padded row is proj_in.bias + x0);  VACE block k is a
 *   main block with its own weights (its own scale_shift_table and its own text k / v among them) on c, with the same timestep_proj
 *   (the r term included), text and RoPE; hint_k = proj_out_k(c) and block k + 1 continues from c, not from the hint.  Behind main
 *   block i, i in vace_layers: x = x + hint * scale with (hint, scale) taken from the FRONT of the list - a block in skip_layers is
 *   passed over before that, so the j-th EXECUTED VACE layer receives hint j with scale j whatever its own index is.
 * VACE block j runs directly before hint j is consumed, and the injection is one token GEMM x + scale_j * (c Wout^T + b): the hint is
 * never materialised, the sum is rounded once, and hints that no executed layer consumes are not computed.
 * Parameter table: fg_wan_create_ex's with `vace_patch_embedding.{weight [D, vace_in_channels, 1, 2, 2], bias}` directly behind
 * `patch_embedding.*` and `vace_blocks.{k}.*` behind the last `blocks.*` key; per VACE block: scale_shift_table, proj_in.{weight,
 * bias} (k = 0 only), the main block's keys in the main block's order, proj_out.{weight, bias}.
 * fp8 mode: the six linears of every VACE block follow the handle's mode, as the main blocks' do (one block body serves both);
 * proj_in (once per context) and proj_out stay bf16 in both modes - the rule is "the six linears of a block", and proj_out has no
 * quantising producer in front of it.
 * FG_EINVAL (the field named): vace_layers not strictly ascending in [0, num_layers), num_vace_layers outside [1, 64],
 * vace_in_channels outside (0, 128].  On such a handle fg_wan_forward_full, fg_wan_forward_full_features, fg_wan_full_sampler_run and
 * fg_wan_full_guided_sampler_run (context set at batch 2 B) work; the chunked and causal entry points return FG_EINVAL.  In
 * fg_wan_forward_full_features tap_blocks may also name num_layers + k: VACE block k, its five taps taken from the control stream
 * (FG_EINVAL when that block does not run under the call's skip_layers, and on every other handle).  fg_wan_set_text also fills the
 * VACE blocks' own text k / v.  fg_wan_pack_group packs a VACE block only when all of its parameters are in the group (they arrive
 * with the root group: the reference's fully_shard wraps `blocks` only); a group that holds some of them is FG_ENOTREADY. */
typedef struct fg_wan_vace_config {
    int vace_in_channels;   /* 96: channels of the control video (inactive | reactive latents | 64 mask channels) */
    int num_vace_layers;
    int vace_layers[64];    /* the main blocks behind which a hint is added, strictly ascending */
} fg_wan_vace_config;
FG_API int fg_wan_create_vace(const fg_wan_config* cfg, const fg_wan_ext_config* ext /* nullable */, const fg_wan_vace_config* vace, fg_wan** out);
/* The hint scales (`context_scale`): n == num_vace_layers host floats, kept on the handle as [n][D] fp32 rows (the gate rows of the
 * injection GEMM) and rewritten in place, so that a captured loop replays with the new scales.  Ones after creation. */
FG_API int fg_wan_set_vace_scale(fg_wan* h, const float* scales_host, int n, void* stream);
/* vid_context [batch, vace_in_channels, ctx_frames, height, width] fp32 (device), ctx_frames <= frames.  Neither the context nor
 * proj_in depends on the step: ctx_in = proj_in(pad(vace_patch_embedding(vid_context))), bf16 [batch, frames * height/2 * width/2, D],
 * is computed once here (padded rows equal the bias, rounded to bf16).  The handle owns it: rewritten in place while the shapes stay
 * (a captured loop replays on the new contents), reallocated otherwise.  Packing weights invalidates it; FG_ENOTREADY before packing,
 * and from a forward without a context of the call's batch, frames and size.  The workspace (256-byte aligned,
 * fg_wan_vace_context_workspace_bytes) is scratch of this call only. */
FG_API size_t fg_wan_vace_context_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width);
FG_API int fg_wan_set_vace_context(fg_wan* h, const float* vid_context, int batch, int frames, int ctx_frames, int height, int width,
                                   void* workspace, size_t workspace_bytes, void* stream);
/* Exposed for the tests: ctx_in as fp32 [batch, frames * height/2 * width/2, D].  FG_ENOTREADY before a context is set. */
FG_API int fg_wan_vace_context_read(fg_wan* h, float* ctx_in_out, void* stream);
/* One step of that solver, in place (misc.hip guided_multistep_kernel): with the eight DEVICE doubles tab = {s, g, c0, c1, c2, p0, p1, p2}
 * each rounded once to fp32, v = guided ? v[total + i] + g (v[i] - v[total + i]) : v[i]; m = x - s v; x_corr = c0 x_last + c1 m_prev +
 * c2 m (first != 0: x_last := x, m_prev := m, neither buffer is read); x_next = p0 x_corr + p1 m_prev + p2 m; then x <- x_next (and
 * x2 <- x_next, nullable), x_last <- x_corr, m_prev <- m.  Every product and sum is an fp32 operation of its own, left to right as
 * written.  v: [2 total] when guided (conditional rows first), else [total].  16-byte accesses when total % 4 == 0 and the pointers
 * allow, else element by element. */
FG_API int fg_op_guided_multistep(const float* v, float* x, float* x2, float* x_last, float* m_prev, const double* tab, int guided, int first,
                                  int64_t total, void* stream);

/* Samples to image bytes, the step after generator_fn in the reference's sample writer
 * (scripts/fid/compute_fid_from_ckpts.py:199): out[n,y,x,c] = uint8(clip(images[n,c,y,x] * 127.5 + 128, 0, 255)),
 * fp32 multiply then add, truncation; NaN -> 0.  images NCHW fp32, out NHWC bytes. */
FG_API int fg_op_images_to_u8(const float* images, uint8_t* out, int64_t batch, int channels, int height, int width,
                       void* stream);
/* Standard normal draws: Philox4x32-10(key = seed, counter = (offset, index/4)) + Box-Muller. */
FG_API int fg_op_randn(float* out, int64_t total, uint64_t seed, uint64_t offset, void* stream);
/* softmax(q k^T / sqrt(head_dim)) v per (batch, head), head_dim 128 or 72, bf16 tensors q / out [batch, lq, heads * head_dim], k / v
 * [batch, lkv, heads * head_dim], fp32 online softmax (wan.hip fa_kernel: the causal video DiT's KV-cache and text attention,
 * fastgen/networks/Wan/network_causal.py:331-412, and DiT-XL/2's 16 x 72 attention, fastgen/networks/DiT/network.py:168,191).
 * Exposed for the parity tests. */
FG_API int fg_op_attention(const void* q, const void* k, const void* v, void* out, int batch, int heads, int head_dim, int lq, int lkv,
                           void* stream);
/* The same with the number of key splits fixed: nsplit 0 = the launcher's cost model (what the networks run), 1 = one workgroup walks
 * all keys of its query tile, 2 .. 8 = that many workgroups share them and a merge pass combines their partial outputs by
 * log-sum-exp.  For the parity tests: the split paths against each other at the video DiT's full sequence lengths. */
FG_API int fg_op_attention_split(const void* q, const void* k, const void* v, void* out, int batch, int heads, int head_dim, int lq, int lkv,
                                 int nsplit, void* stream);
/* The kernel forms of token attention (wan.hip): what fg_attention_plan.kernel names and what `path` selects. */
#define FG_FA_TILE128 1     /* fa_kernel<128, 2, true>: 128-query tiles, LDS-DMA ring (the launcher's choice below 1024 keys) */
#define FG_FA_TILE128_W3 2  /* fa_kernel<128, 3, true>: the same compiled for three waves per SIMD (FASTGEN_AMD_FA_WAVES=3) */
#define FG_FA_TILE128_REG 3 /* fa_kernel<128, 2, false>: register prefetch instead of LDS-DMA (FASTGEN_AMD_FA_DMA=0) */
#define FG_FA_WIDE 4        /* fa2_kernel, 256-query tiles, even key splits (>= 1024 keys; FASTGEN_AMD_FA_WIDE=1, FASTGEN_AMD_FA_CUT=0) */
#define FG_FA_WIDE_CUT 5    /* fa2_kernel with the uneven two-way cut at key tile t_cut (grids of fewer workgroups than CUs) */
#define FG_FA_SEQ72 6       /* fa72_seq_kernel: head dim 72, at most 256 keys, all of them in one pass */
#define FG_FA_TILE72 7      /* fa_kernel<72, 2, false> (FASTGEN_AMD_FA_SEQ72=0, more than 256 keys or a forced split) */
#define FG_FA_TILE72_W3 8   /* fa_kernel<72, 3, false> (FASTGEN_AMD_FA_WAVES=3) */
#define FG_FA_REFUSE_ARG 1    /* bad argument (head_dim, a count <= 0, ldk % 8, force_split out of [0, 8] or > 1 without scratch) */
#define FG_FA_REFUSE_OFFSET 2 /* head dim 128: lkv * ldk * 2 bytes do not fit the kernels' 32-bit buffer offsets */
#define FG_FA_REFUSE_PATH 3   /* the kernel form `path` names cannot serve this shape (it is never redirected to another) */
typedef struct fg_attention_plan {
    int kernel;           /* FG_FA_* */
    int nsplit;           /* key splits; > 1: partial outputs in scratch + the merge pass */
    int t_cut;            /* FG_FA_WIDE_CUT: the pieces are key tiles [0, t_cut) and [t_cut, ceil(lkv / 32)); else 0 */
    int sample_major;     /* workgroup map: all heads of a sample on one XCD (batch >= 8, lq <= 1024, one split; FG_FA_SEQ72 always) */
    int refusal;          /* 0 or FG_FA_REFUSE_*: the other members are then zero */
    int64_t grid;         /* workgroups of the attention kernel */
    size_t scratch_bytes; /* what use_scratch allocates: room for 8 splits' fp32 partial outputs and log-sum-exps */
} fg_attention_plan;
/* What token attention would launch for this shape: the launcher's decisions and nothing else (no launch, no GPU needed).  ldk: row
 * pitch of k / v in elements; use_scratch 0: never split; force_split as fg_op_attention_split's nsplit; path 0: the launcher's own
 * choice (the FASTGEN_AMD_FA_* switches, read once per process, included), FG_FA_*: that form or refusal FG_FA_REFUSE_PATH.
 * Returns FG_OK with *plan filled, refusals included. */
FG_API int fg_op_attention_plan(int head_dim, int batch, int heads, int lq, int lkv, int ldk, int use_scratch, int force_split, int path,
                                fg_attention_plan* plan);
/* The DiT engine's attention (dit.hip) on its own operand layouts: q, k [batch][heads][tokens][head_dim], vt [batch][heads][head_dim][tokens]
 * followed by 32 rows (32 * tokens elements) of readable slack, out [batch][tokens][heads * head_dim].  mode FG_DTYPE_BF16: bf16 tensors;
 * FG_DTYPE_BF16X3: q / k / vt are a hi and a lo bf16 plane each, lo_off elements apart, out fp32.  head_dim 64 or 72; tokens a multiple
 * of 256.  path 0: what fg_dit_forward launches (256 tokens: the whole-sequence kernel, bit-identical to path 1; otherwise the flash
 * form), 1: the whole-sequence kernel (256 tokens only), 2: the flash form (online softmax over blocks of 128 keys).  A path that cannot
 * serve the shape is FG_EINVAL and launches nothing.  For the per-element parity tests and scripts/attn_bench.py. */
FG_API int fg_op_dit_attention(int mode, const void* q, const void* k, const void* vt, void* out, int batch, int heads, int head_dim,
                               int tokens, size_t lo_off, int path, void* stream);
/* fg_op_attention on the layouts the engines pass: q / k / v / out rows of ldq / ldk / ldk / ldo elements (head h at column
 * h * head_dim), q_bs / kv_bs / o_bs elements between samples - packed q|k|v rows (ldq = ldk = 3 D, v = k + D), interleaved k|v
 * (ldk = 2 D), a KV cache whose kv_bs exceeds lkv * ldk.  ldq % 8 == ldk % 8 == ldo % 4 == 0, 16-byte aligned q / k / v, 8-byte out.
 * use_scratch, force_split, path as in fg_op_attention_plan; a refused plan is FG_EINVAL with its reason in fg_last_error().
 * fg_op_attention(_split) is this call with contiguous tensors, scratch and path 0.  For the per-element parity tests. */
FG_API int fg_op_attention_ex(const void* q, int ldq, int64_t q_bs, const void* k, const void* v, int ldk, int64_t kv_bs, void* out, int ldo,
                              int64_t o_bs, int batch, int heads, int head_dim, int lq, int lkv, int use_scratch, int force_split, int path,
                              void* stream);
/* The cross-attention of an image-to-video block (wan_i2v.hip wan_dual_xattn_kernel), head dim 128, on the layouts of
 * fg_op_attention_ex: out = softmax(q k_txt^T / sqrt(128)) v_txt + softmax(q k_img^T / sqrt(128)) v_img - two independent softmaxes,
 * each output rounded to bf16, their fp32 sum rounded to bf16.  Either key count may be ragged; nothing is read past key l_txt - 1 /
 * l_img - 1.  l_img == 0 (k_img / v_img then unread): the text attention alone, bit-identical to fg_op_attention_ex without scratch.
 * For the per-element parity test and scripts/attn_bench.py. */
FG_API int fg_op_wan_dual_cross_attention(const void* q, int ldq, int64_t q_bs, const void* k_txt, const void* v_txt, int ldk_txt,
                                          int64_t kv_bs_txt, int l_txt, const void* k_img, const void* v_img, int ldk_img, int64_t kv_bs_img,
                                          int l_img, void* out, int ldo, int64_t o_bs, int batch, int heads, int lq, void* stream);
/* The two ends of the video DiT on their own (wan_embed.hip; wan.hip / wan_ti2v.hip), for the per-element tests and timing.  first_frame
 * (nullable) [batch, channels, 1, height, width]: the second source - frame 0's tokens are computed from it / frame 0 of the head's
 * result is its copy.  path 0: what the engine launches (channels == 48: the phased embedding of wan_embed.hip, the tiled head of
 * wan_ti2v.hip; 16 channels without a second source: the rows-in-registers embedding), 1: the per-output embedding / the
 * wave-per-token head of wan.hip, 2: the 48-channel kernels, FG_EINVAL where they do not apply.  The embedding kernels are bit-identical.
 * fg_op_wan_patch_embed: x [batch, channels, frames, height, width] fp32, w [d, channels, 1, 2, 2], bias [d] -> tokens bf16
 * [batch, frames * height/2 * width/2, d].  fg_op_wan_final: tokens bf16 [batch * frames * gh * gw, d], mod [batch * frames][2][d]
 * {shift, scale}, w [4 * channels, d], bias [4 * channels] -> out fp32 [batch, channels, frames, 2 gh, 2 gw]; d in {256, 384, 1536,
 * 2048, 3072, 5120} for the head of wan.hip, d % 32 == 0 for the tiled one. */
FG_API int fg_op_wan_patch_embed(const float* x, const float* first_frame, const float* w, const float* bias, void* out, int batch, int channels,
                                 int frames, int height, int width, int d, int path, void* stream);
FG_API int fg_op_wan_final(const void* tokens, const float* mod, const float* w, const float* bias, const float* first_frame, float* out, int batch,
                           int channels, int frames, int gh, int gw, int d, float eps, int path, void* stream);
/* The control branch's patch embedding on its own (wan_embed.hip): fg_op_wan_patch_embed's arithmetic for up to 128 channels, without a
 * second source.  path 0: what fg_wan_set_vace_context launches (channels == 96: the phased kernel), 1: the per-output kernel,
 * 2: the phased kernel, FG_EINVAL unless channels == 96.  The two are bit-identical (one fmaf chain per output). */
FG_API int fg_op_wan_vace_patch_embed(const float* x, const float* w, const float* bias, void* out, int batch, int channels, int frames, int height,
                                      int width, int d, int path, void* stream);
/* The transformer blocks' token GEMM in the bf16 compute mode (gemm.hip; reference: the nn.Linear calls of DiTBlock,
 * fastgen/networks/DiT/network.py:168-198, under bf16 autocast): out[m][n] = resid[m][n] + gate[(m / gate_rows) * gate_stride + n] *
 * act(sum_k a[m][k] w[n][k] + bias[n]) with a [m][k], w [n][k], resid / out [m][n] in bf16, fp32 accumulation, bias / gate fp32;
 * act 0 none, 1 GELU(tanh) (anything else: FG_EINVAL); bias, gate, resid nullable.  k % 64 == 0, n % 16 == 0.  tile_order: 0 linear, 1 XCD-aware (launcher's
 * choice), 2 / 4 / 8 XCD columns over n; + 16 forces the register-staged kernel, + 32 the LDS-DMA ping-pong kernel (default: the
 * latter where m, n >= 256), + 256 its narrow-tile form (256 x 128: what short token counts - one sample of the video DiT - take),
 * + 64 lets grids of fewer tiles than half the CUs split K (fp32 partial sums + a finishing pass); bits 16, 32 and 256 exclude each
 * other.  What a call launches: fg_op_gemm_plan.  Exposed for the parity tests and scripts/gemm_bench.py. */
FG_API int fg_op_gemm_bf16(const void* a, const void* w, const float* bias, void* out, int m, int n, int k, int act, const float* gate,
                           int gate_stride, int gate_rows, const void* resid, int tile_order, void* stream);
/* The kernel forms and epilogues of the token GEMM (gemm.hip): what fg_gemm_plan names. */
#define FG_GEMM_REG 1       /* gemm_bf16_kernel: register-staged, tiles of 256 tokens x 256 | 192 outputs */
#define FG_GEMM_PP 2        /* gemm_bf16_pp_kernel: LDS-DMA, two ping-pong wave groups, 256 x 256 (m, n >= 256) */
#define FG_GEMM_PP_NARROW 3 /* gemm_bf16_pp2_kernel: its 256 x 128 form (short grids; tile_order + 256) */
#define FG_GEMM_PP_SPLITK 4 /* gemm_bf16_pp_kernel over ksplit pieces of k (fp32 partial sums in scratch) + gemm_splitk_finish_kernel */
#define FG_GEMM_EPI_TOK 0     /* bf16 out [m][n]: bias, act, gate x value + resid */
#define FG_GEMM_EPI_HEADS 1   /* bf16 q | k | v^T split by head (the qkv linear) */
#define FG_GEMM_EPI_RAW 2     /* fp32 partial sums (FG_GEMM_PP_SPLITK; the finishing pass applies FG_GEMM_EPI_TOK) */
#define FG_GEMM_EPI_TOK32 3   /* fp32 out [m][n] */
#define FG_GEMM_EPI_SPLIT 4   /* [hi | lo] bf16 planes [m][2 n] of the fp32 value (split-bf16, out_mode 1) */
#define FG_GEMM_EPI_HEADS32 5 /* head-split hi / lo planes (split-bf16 qkv) */
/* FG_GEMM_REFUSE_ARG, a bad argument: a count <= 0, k % 64 (fp8: 128), n % 16, heads that do not divide n, a tile_order / out_mode the
 * flavour does not take, split-bf16 below m = 256 or n = 256, piece >= pieces */
#define FG_GEMM_REFUSE_ARG 1
#define FG_GEMM_REFUSE_OFFSET 2 /* w, or one 256-row tile of a / out, does not fit the kernels' 32-bit buffer offsets (2 GiB) */
#define FG_GEMM_REFUSE_FORM 3   /* fp32 out, or the fp8 head split, where the ping-pong kernel cannot run (it alone has those epilogues) */
#define FG_GEMM_REFUSE_PIECE 4  /* split-bf16: the row cutting leaves a last launch of fewer than 256 rows */
typedef struct fg_gemm_plan {
    int refusal;   /* 0 or FG_GEMM_REFUSE_*: the whole call is refused, the other members are zero */
    int kernel;    /* FG_GEMM_* */
    int tile_n;    /* outputs per tile: 256, 192 or 128 (tokens per tile: always 256) */
    int epilogue;  /* FG_GEMM_EPI_* */
    int ksplit;    /* pieces of k per tile (1 unless FG_GEMM_PP_SPLITK) */
    int xn;        /* tile order as the kernel sees it: 0 linear, else the 8 XCDs form (8 / xn) x xn over (token, output) tiles */
    int grid;      /* workgroups, at most cus; each walks the work items (tile, k piece) first, first + stride, ... */
    int lds_bytes; /* dynamic LDS per workgroup */
    int row0, rows; /* this piece: rows [row0, row0 + rows) of the call */
    int pieces;    /* launches the call is cut into so that byte offsets into a / out / resid stay below 2 GiB */
} fg_gemm_plan;
/* What the token GEMM would launch for row piece `piece` of a call: the launcher's decisions and nothing else (no launch, no GPU
 * needed).  flavour 0: fg_op_gemm_bf16 (out_mode 1: fp32 out, an option of the engines), 1: fg_op_gemm_x3 (k its real k; out_mode as
 * there; tile_order 0 .. 15), 2: fg_op_gemm_fp8 (out_mode 0).  heads > 0: the head-split epilogue of the qkv linear (n = 3 heads
 * head_dim); gate_rows 0: no gate; scratch_bytes: split-K scratch the caller has (tile_order + 64 counts as the 16 m n bytes
 * fg_op_gemm_bf16 allocates); tile_order as the flavour's entry point takes it; cus: compute units of the device.  The switches
 * FASTGEN_AMD_GEMM_PP / FASTGEN_AMD_GEMM_NARROW, read once per process, are part of the plan.  Returns FG_OK with *plan filled,
 * refusals included. */
FG_API int fg_op_gemm_plan(int flavour, int m, int n, int k, int heads, int gate_rows, size_t scratch_bytes, int tile_order, int out_mode,
                           int cus, int piece, fg_gemm_plan* plan);
/* Row quantiser of the fp8 compute mode (gemm.hip): x [m][k] fp32 (dtype 0) or bf16 (dtype 1) -> q [m][k] OCP e4m3fn bytes and
 * scale [m] fp32.  Per row: amax = max |x|; amax == 0: scale = 1 and q = 0; else scale = amax / 448.0f, q = e4m3fn_RNE(clamp(x *
 * (448.0f / amax), -448, 448)) (IEEE fp32 divisions and product).  k % 128 == 0; anything else: FG_EINVAL before any launch. */
FG_API int fg_op_quant_rows_fp8(int dtype, const void* x, void* q, float* scale, int64_t m, int k, void* stream);
/* The token GEMM on e4m3fn operands (FG_DTYPE_FP8; gemm.hip, v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales):
 * out[m][n] = resid[m][n] + gate[(m / gate_rows) * gate_stride + n] * act(a_scale[m] * w_scale[n] * sum_k a[m][k] w[n][k] + bias[n])
 * with a [m][k], w [n][k] e4m3fn bytes (fg_op_quant_rows_fp8), a_scale [m], w_scale [n], bias, gate fp32, resid / out bf16, fp32
 * accumulation; act 0 none, 1 GELU(tanh); bias, gate, resid nullable.  m >= 1, n % 16 == 0, k % 128 == 0, n k < 2^31; anything else:
 * FG_EINVAL before any launch.  tile_order: 0 linear, 1 XCD-aware, 2 / 4 / 8 XCD columns over n; + 16 forces the register-staged
 * kernel (default: the LDS-DMA ping-pong kernel where m, n, k >= 256).  Exposed for the parity tests and scripts/gemm_bench.py. */
FG_API int fg_op_gemm_fp8(const void* a, const void* w, const float* bias, void* out, int m, int n, int k, int act, const float* gate,
                          int gate_stride, int gate_rows, const void* resid, int tile_order, const float* a_scale, const float* w_scale,
                          void* stream);
/* LayerNorm (eps 1e-6, no affine) + adaLN modulation with the quantising store of the fp8 mode (dit.hip): y = LN(x[tok]) * (1 +
 * mod[n][scale_off + c]) + mod[n][shift_off + c], n = tok / tokens_per_image, written as e4m3fn bytes y [ntok][d] + y_scale [ntok]
 * (the scheme of fg_op_quant_rows_fp8 applied to the fp32 y).  x bf16 [ntok][d]; d in {384, 768, 1024, 1152} (DiT) or {256, 1536,
 * 2048, 3072, 5120} (the causal video DiT, tokens_per_image = tokens per frame); mod_stride and the offsets multiples of 4. */
FG_API int fg_op_dit_ln_modulate_fp8(const void* x, const float* mod, int mod_stride, int shift_off, int scale_off, void* y, float* y_scale,
                                     int ntok, int d, int tokens_per_image, void* stream);
/* The same token GEMM in the split-bf16 (FG_DTYPE_BF16X3) mode, the DiT's default: a [m][k] and w [n][k] fp32 are split into bf16
 * hi / lo planes (scratch allocated here, freed once the stream has drained: a test entry point, not a hot path) and contracted as
 * a_hi w_hi + a_hi w_lo + a_lo w_hi with fp32 accumulation; out[m][n] = resid[m][n] + gate[(m / gate_rows) * gate_stride + n] *
 * act(... + bias[n]) in fp32.  out_mode 0: out fp32 [m][n] (out may alias resid); 1: out [m][2 n] bf16, row r = [hi | lo] of the
 * fp32 value.  act 0 none, 1 GELU(tanh); bias, gate, resid nullable (fp32; every pointer 16-byte aligned; gate_stride a multiple of 4, >= n).
 * m >= 256, n >= 256, n % 16 == 0, k % 64 == 0, n * 3 k * 2 < 2^31; anything else: FG_EINVAL before any launch. */
FG_API int fg_op_gemm_x3(const float* a, const float* w, const float* bias, void* out, int m, int n, int k, int act, const float* gate,
                         int gate_stride, int gate_rows, const float* resid, int out_mode, void* stream);

/* ================================ EDM2 U-Net (EDM2Precond, reference fastgen/networks/EDM2/network.py) ================================
 * The magnitude-preserving ImageNet-64 network of the EDM2 consistency-model recipes, forward and few-step sampling only.  A handle of
 * its own: EDM2's knobs (balances, clipping, gains, Fourier buffers) are not fg_edm_config fields.  Activations are fp32 NHWC inside;
 * the convolutions run in FG_DTYPE_BF16X3 or FG_DTYPE_BF16.  Supported envelope (checked by fg_edm2_create, FG_EINVAL otherwise):
 * img_resolution 8 .. 64 (power of two), img_channels 1 .. 4, every level width a multiple of 64, attention at resolutions >= 8 with
 * 64-channel heads, lowest resolution >= 8. */
typedef struct fg_edm2_config {
    int img_resolution;                  /* 64 */
    int img_channels;                    /* 3 */
    int label_dim;                       /* 1000 (0 = unconditional) */
    int model_channels;                  /* 192 (S) / 384 (XL) */
    int num_levels;                      /* len(channel_mult) */
    int channel_mult[FG_MAX_LEVELS];     /* {1,2,3,4} */
    int channel_mult_noise;              /* 0 = None: noise embedding width = the first level's width */
    int channel_mult_emb;                /* 0 = None: embedding width = the widest level's width */
    int num_blocks;                      /* 3 */
    int num_attn_resolutions;
    int attn_resolutions[FG_MAX_LEVELS]; /* {16, 8} */
    double label_balance;                /* 0.5 */
    double concat_balance;               /* 0.5 */
    double res_balance;                  /* 0.3 */
    double attn_balance;                 /* 0.3 */
    double clip_act;                     /* 256 (<= 0: no clipping) */
    double sigma_data;                   /* 0.5 */
    double sigma_shift;                  /* 0.0 (applied in eval mode only: see fg_edm2_set_training) */
    int compute_dtype;                   /* FG_DTYPE_BF16X3 or FG_DTYPE_BF16 */
    int drop_precond;                    /* bit mask of FG_DROP_PRECOND_* */
} fg_edm2_config;

typedef struct fg_edm2 fg_edm2; /* opaque */

FG_API int fg_edm2_create(const fg_edm2_config* cfg, fg_edm2** out);
FG_API void fg_edm2_destroy(fg_edm2* h);
/* The engine's parameters in the reference's state_dict() order with its names ("unet.out_gain", "unet.emb_fourier.freqs",
 * "unet.emb_fourier.phases", "unet.emb_noise.weight", ...): every weight-carrying entry of the U-Net plus the two Fourier buffers.
 * The logvar head (logvar_fourier, logvar_linear) is not part of the engine. */
FG_API int fg_edm2_num_params(const fg_edm2* h);
FG_API int fg_edm2_param_info(const fg_edm2* h, int index, const char** name, int* ndim, int64_t shape[4]);
/* Borrow a device fp32 tensor for a parameter (raw, un-normalised weights, as the module holds them). */
FG_API int fg_edm2_bind_param(fg_edm2* h, const char* name, const float* device_ptr, int64_t numel);
/* Normalise and pack every weight from the bound tensors: w / (1e-4 + |w_o| / sqrt(fan_in)) * gain / sqrt(fan_in) per output row,
 * with mp_silu's 1/0.596 and mp_sum's / mp_cat's constant weights folded in.  Must run again after any bound tensor changed, the
 * gains (emb_gain, out_gain) included. */
FG_API int fg_edm2_pack_weights(fg_edm2* h, void* stream);
FG_API size_t fg_edm2_workspace_bytes(const fg_edm2* h, int batch);
/* EDM2Precond.forward in eval mode with fwd_pred_type = 'x0': x_t / out NCHW fp32 [B, C, R, R], t fp64 [B], class_labels fp32
 * [B, label_dim] or NULL (= zeros).  emb_out (nullable): the embedding mp_silu(...) [B, emb_channels]. */
FG_API int fg_edm2_forward(fg_edm2* h, const float* x_t, const double* t, const float* class_labels, float* out, float* emb_out,
                           int batch, void* workspace, size_t workspace_bytes, void* stream);
/* Exposed for the parity tests (tests/test_gpu_edm2_ops.py): fg_edm2_forward with taps - the same forward, the same launches, fp32 copies
 * on `stream` behind the kernels that wrote the buffers; `out` and `emb_out` are what the untapped call leaves, bit for bit.  taps: HOST
 * array of num_taps = fg_edm2_num_taps(h) = 2 + fg_edm2_num_blocks(h) device buffers, each nullable, fp32 NHWC: taps[0] the stem conv's
 * output [B, R, R, width of level 0]; taps[1 + i] the output of block i in fg_edm2_block_info order [B, res_out, res_out, cout];
 * taps[num_taps - 1] the raw U-Net output F [B, R, R, img_channels] (before precond_output).  taps NULL: fg_edm2_forward.  Another
 * num_taps, or a tap that aliases x_t / out / emb_out: FG_EINVAL. */
FG_API int fg_edm2_num_taps(const fg_edm2* h);
FG_API int fg_edm2_forward_taps(fg_edm2* h, const float* x_t, const double* t, const float* class_labels, float* out, float* emb_out,
                                float* const* taps, int num_taps, int batch, void* workspace, size_t workspace_bytes, void* stream);
/* train() / eval(): sigma_shift applies in eval mode only (training != 0 disables it). */
FG_API int fg_edm2_set_training(fg_edm2* h, int training);
/* The FG_LOOP_X0 student loop of fg_sampler_run (same arguments, checks and semantics, EDM schedule) around fg_edm2_forward;
 * use_graph != 0 replays one cached hipGraph per (batch, steps, sample type, pointers) key. */
FG_API int fg_edm2_sampler_run(fg_edm2* h, const float* noise, const float* class_labels, const double* t_list, int steps,
                               int sample_type, int loop_kind, const float* eps, uint64_t seed, float* out, int batch,
                               void* workspace, size_t workspace_bytes, int use_graph, void* stream);
/* The U-Net's Blocks, encoder then decoder (not the stem conv or out_conv): key "unet.enc.<res>x<res>_<name>" / "unet.dec....",
 * res_in = 2 res_out for a down block, res_out / 2 for an up block.  run_block runs one on NHWC fp32 tensors with emb [B, emb_channels]
 * (the mp_silu output).  A decoder block with a skip takes the two raw producers (x1: the main path, c1 channels; x2: the popped skip,
 * c2 channels) and applies mp_cat itself; any other (c1, c2) split is FG_EINVAL before anything runs. */
FG_API int fg_edm2_num_blocks(const fg_edm2* h);
FG_API int fg_edm2_block_info(const fg_edm2* h, int index, const char** key, int* cin, int* cout, int* res_in, int* res_out,
                              int* has_attention);
FG_API int fg_edm2_run_block(fg_edm2* h, int index, const float* x1, int c1, const float* x2, int c2, const float* emb, float* out,
                             int batch, void* workspace, size_t workspace_bytes, void* stream);
/* Forward-mode derivative of fg_edm2_forward along (vx [B, C, R, R], vt fp32 [B] or NULL = 0) - what torch.func.jvp of
 * EDM2Precond.forward(x_t, t) returns: out = fg_edm2_forward's output, bit for bit (the same kernels in the same order), jvp its
 * directional derivative, both NCHW fp32.  The primal and the tangent run block by block, interleaved; the compute mode applies to the
 * convolutions of both, everything else is fp32.  The clamp's tangent is 0 where the clamped activation has |y| >= clip_act
 * (torch passes it where the unclamped value equals +-clip_act exactly).  Workspace: fg_edm2_jvp_workspace_bytes (256-byte aligned); a
 * smaller one is FG_EINVAL.  Arguments are checked before anything is launched. */
FG_API size_t fg_edm2_jvp_workspace_bytes(const fg_edm2* h, int batch);
FG_API int fg_edm2_jvp(fg_edm2* h, const float* x_t, const double* t, const float* class_labels, const float* vx, const float* vt,
                       float* out, float* jvp, int batch, void* workspace, size_t workspace_bytes, void* stream);
/* fg_edm2_run_block with tangents (x1_d, x2_d, emb_d -> out_d): workspace of fg_edm2_jvp_workspace_bytes. */
FG_API int fg_edm2_run_block_jvp(fg_edm2* h, int index, const float* x1, const float* x1_d, int c1, const float* x2, const float* x2_d,
                                 int c2, const float* emb, const float* emb_d, float* out, float* out_d, int batch, void* workspace,
                                 size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FASTGEN_AMD_H */
