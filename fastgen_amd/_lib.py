"""ctypes binding of libfastgen_amd.so (C ABI: include/fastgen_amd.h).  There is no fallback: if the library is
missing or a call fails, this raises."""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfastgen_amd.so")

FG_MAX_LEVELS = 8
FG_DTYPE_F32, FG_DTYPE_BF16, FG_DTYPE_BF16X3, FG_DTYPE_FP8 = 0, 1, 2, 3
DTYPE_NAMES = {"fp32": FG_DTYPE_F32, "bf16": FG_DTYPE_BF16, "bf16x3": FG_DTYPE_BF16X3, "fp8": FG_DTYPE_FP8}
FG_SAMPLE_SDE, FG_SAMPLE_ODE = 0, 1
SAMPLE_TYPES = {"sde": FG_SAMPLE_SDE, "ode": FG_SAMPLE_ODE}
FG_LOOP_X0, FG_LOOP_MEANFLOW, FG_LOOP_EULER = 0, 1, 2
LOOP_KINDS = {"x0": FG_LOOP_X0, "meanflow": FG_LOOP_MEANFLOW, "euler": FG_LOOP_EULER}
FG_SCHEDULE_EDM, FG_SCHEDULE_RF = 0, 1
FG_DROP_PRECOND_INPUT, FG_DROP_PRECOND_OUTPUT = 1, 2
FG_BWD_DECODER, FG_BWD_ENCODER, FG_BWD_EMBED = 1, 2, 4
FG_MODEL_SONGUNET, FG_MODEL_DHARIWAL = 0, 1
(FG_TRAIN_OP_HEAD_GRAD, FG_TRAIN_OP_STEM_OPERAND, FG_TRAIN_OP_INPUT_GRAD, FG_TRAIN_OP_ADD_NCHW_TO_NHWC, FG_TRAIN_OP_SILU_BWD, FG_TRAIN_OP_JVP_COEF,
 FG_TRAIN_OP_JVP_EMBED, FG_TRAIN_OP_JVP_INPUT, FG_TRAIN_OP_JVP_OUTPUT) = range(9)  # fg_op_train_elementwise


class fg_edm_config(ctypes.Structure):
    _fields_ = [
        ("img_resolution", c_int), ("img_channels", c_int), ("label_dim", c_int), ("augment_dim", c_int),
        ("model_channels", c_int), ("num_levels", c_int), ("channel_mult", c_int * FG_MAX_LEVELS),
        ("channel_mult_emb", c_int), ("num_blocks", c_int), ("num_attn_resolutions", c_int),
        ("attn_resolutions", c_int * FG_MAX_LEVELS), ("channel_mult_noise", c_int), ("sigma_data", c_double),
        ("sigma_shift", c_double), ("compute_dtype", c_int), ("r_timestep", c_int), ("drop_precond", c_int),
        ("schedule", c_int), ("model_type", c_int),
    ]


class fg_edm2_config(ctypes.Structure):
    _fields_ = [
        ("img_resolution", c_int), ("img_channels", c_int), ("label_dim", c_int), ("model_channels", c_int), ("num_levels", c_int),
        ("channel_mult", c_int * FG_MAX_LEVELS), ("channel_mult_noise", c_int), ("channel_mult_emb", c_int), ("num_blocks", c_int),
        ("num_attn_resolutions", c_int), ("attn_resolutions", c_int * FG_MAX_LEVELS), ("label_balance", c_double),
        ("concat_balance", c_double), ("res_balance", c_double), ("attn_balance", c_double), ("clip_act", c_double),
        ("sigma_data", c_double), ("sigma_shift", c_double), ("compute_dtype", c_int), ("drop_precond", c_int),
    ]


class fg_dit_config(ctypes.Structure):
    _fields_ = [("input_size", c_int), ("patch_size", c_int), ("in_channels", c_int), ("hidden_size", c_int), ("depth", c_int),
                ("num_heads", c_int), ("mlp_hidden", c_int), ("embedding_rows", c_int), ("r_timestep", c_int), ("compute_dtype", c_int)]


class fg_wan_config(ctypes.Structure):
    _fields_ = [("num_heads", c_int), ("head_dim", c_int), ("in_channels", c_int), ("out_channels", c_int), ("text_dim", c_int),
                ("freq_dim", c_int), ("ffn_dim", c_int), ("num_layers", c_int), ("rope_max_seq_len", c_int), ("chunk_size", c_int),
                ("total_num_frames", c_int), ("eps", c_float), ("compute_dtype", c_int)]


class fg_wan_ext_config(ctypes.Structure):
    _fields_ = [("r_timestep", c_int), ("time_cond_diff", c_int)]


class fg_wan_i2v_config(ctypes.Structure):
    _fields_ = [("latent_channels", c_int), ("mask_channels", c_int), ("image_dim", c_int)]


class fg_wan_ti2v_config(ctypes.Structure):
    _fields_ = [("latent_channels", c_int)]


class fg_wan_vace_config(ctypes.Structure):
    _fields_ = [("vace_in_channels", c_int), ("num_vace_layers", c_int), ("vace_layers", c_int * 64)]


class fg_wan_block_taps(ctypes.Structure):
    _fields_ = [("attn1", c_void_p), ("x_attn1", c_void_p), ("attn2", c_void_p), ("x_attn2", c_void_p), ("x_ffn", c_void_p)]


class fg_dit_sampler_config(ctypes.Structure):
    _fields_ = [("t_scale", c_double), ("guidance_scale", c_double), ("use_sit_convention", c_int), ("time_cond_diff", c_int),
                ("net_pred_flow", c_int), ("schedule", c_int)]


class fg_wan_sampler_config(ctypes.Structure):
    _fields_ = [("t_scale", c_double), ("context_noise", c_double), ("net_pred_flow", c_int), ("schedule", c_int), ("prefill_frames", c_int)]


class fg_wan_guided_sampler_config(ctypes.Structure):
    _fields_ = [("t_scale", c_double), ("context_noise", c_double), ("guidance", c_int)]


class fg_attention_plan(ctypes.Structure):
    _fields_ = [("kernel", c_int), ("nsplit", c_int), ("t_cut", c_int), ("sample_major", c_int), ("refusal", c_int), ("grid", c_int64),
                ("scratch_bytes", c_size_t)]


class fg_edm_conv_plan(ctypes.Structure):
    _fields_ = [("kernel", c_int), ("stat_slots", c_int)]


# fg_op_edm_conv_pack layouts, fg_edm_conv_plan.kernel, fg_op_edm_head_pack_bytes
FG_EDM_PACK_GENERIC, FG_EDM_PACK_WS, FG_EDM_PACK_X3WS, FG_EDM_PACK_X3SUB = range(4)
FG_EDM_CONV_GENERIC, FG_EDM_CONV_WS, FG_EDM_CONV_X3WS = 1, 2, 3
FG_EDM_PACK_STEM, FG_EDM_PACK_AUX = 0, 1


class fg_gemm_plan(ctypes.Structure):
    _fields_ = [("refusal", c_int), ("kernel", c_int), ("tile_n", c_int), ("epilogue", c_int), ("ksplit", c_int), ("xn", c_int), ("grid", c_int),
                ("lds_bytes", c_int), ("row0", c_int), ("rows", c_int), ("pieces", c_int)]


# token attention's kernel forms (fg_attention_plan.kernel, the `path` argument) and refusal codes
FG_FA_TILE128, FG_FA_TILE128_W3, FG_FA_TILE128_REG, FG_FA_WIDE, FG_FA_WIDE_CUT, FG_FA_SEQ72, FG_FA_TILE72, FG_FA_TILE72_W3 = range(1, 9)
FG_FA_REFUSE_ARG, FG_FA_REFUSE_OFFSET, FG_FA_REFUSE_PATH = 1, 2, 3
# the token GEMM's kernel forms, epilogues and refusal codes (fg_gemm_plan)
FG_GEMM_REG, FG_GEMM_PP, FG_GEMM_PP_NARROW, FG_GEMM_PP_SPLITK = range(1, 5)
FG_GEMM_EPI_TOK, FG_GEMM_EPI_HEADS, FG_GEMM_EPI_RAW, FG_GEMM_EPI_TOK32, FG_GEMM_EPI_SPLIT, FG_GEMM_EPI_HEADS32 = range(6)
FG_GEMM_REFUSE_ARG, FG_GEMM_REFUSE_OFFSET, FG_GEMM_REFUSE_FORM, FG_GEMM_REFUSE_PIECE = 1, 2, 3, 4


# name -> (restype, argtypes); every symbol include/fastgen_amd.h declares
SIGNATURES = {
    "fg_last_error": (c_char_p, []),
    "fg_version": (c_char_p, []),
    "fg_graph_stats": (None, [POINTER(c_uint64), POINTER(c_uint64)]),
    "fg_edm_create": (c_int, [POINTER(fg_edm_config), POINTER(c_void_p)]),
    "fg_edm_destroy": (None, [c_void_p]),
    "fg_edm_num_params": (c_int, [c_void_p]),
    "fg_edm_param_info": (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_int), POINTER(c_int64)]),
    "fg_edm_bind_param": (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    "fg_edm_pack_weights": (c_int, [c_void_p, c_void_p]),
    "fg_edm_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "fg_edm_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                               c_size_t, c_void_p]),
    "fg_edm_num_feature_taps": (c_int, [c_void_p]),
    "fg_edm_feature_info": (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_int), POINTER(c_int)]),
    "fg_edm_forward_features": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p), c_int,
                                        c_void_p, c_size_t, c_void_p]),
    "fg_sampler_run": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_double), c_int, c_int, c_int, c_void_p, c_uint64,
                               c_void_p, c_int, c_void_p, c_size_t, c_int, c_void_p]),
    "fg_edm_t_list": (c_int, [c_int, POINTER(c_double)]),
    "fg_rf_t_list": (c_int, [c_int, POINTER(c_double)]),
    "fg_edm_profile_begin": (c_int, [c_void_p]),
    "fg_edm_profile_end": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_double), POINTER(c_double)]),
    "fg_edm_num_blocks": (c_int, [c_void_p]),
    "fg_edm_block_info": (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_int), POINTER(c_int), POINTER(c_int),
                                  POINTER(c_int), POINTER(c_int)]),
    "fg_edm_run_block": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                 c_size_t, c_void_p]),
    "fg_op_gn_coeffs": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_void_p]),
    "fg_op_adm_conv_pack_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "fg_op_adm_conv_pack": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fg_op_adm_conv": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                               c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "fg_op_adm_conv_ex": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                                  c_void_p, c_void_p, c_int, c_float, c_float, c_void_p, c_int, c_void_p]),
    "fg_op_adm_gn_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "fg_op_adm_gn_coeffs": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p, c_int,
                                    c_int, c_void_p, c_size_t, c_void_p]),
    "fg_op_adm_attention": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fg_op_edm2_attention": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fg_op_edm2_prep_weight": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_float, c_float, c_int, c_void_p]),
    "fg_op_edm2_pixel_norm": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_edm2_attention_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fg_op_edm2_pixel_norm_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_edm2_silu_operand_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                            c_int, c_int, c_void_p]),
    "fg_op_linear": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_adm_map_in": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "fg_op_latents": (c_int, [c_void_p, c_double, c_void_p, c_int64, c_void_p]),
    "fg_op_forward_process": (c_int, [c_void_p, c_void_p, c_double, c_int, c_void_p, c_int64, c_void_p]),
    "fg_op_x0_to_eps": (c_int, [c_void_p, c_void_p, c_double, c_int, c_void_p, c_int64, c_void_p]),
    "fg_op_conv_wgrad_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "fg_op_conv_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, ctypes.c_size_t, c_void_p]),
    "fg_op_conv_wgrad_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, ctypes.c_size_t, c_void_p]),
    "fg_edm_bind_grad": (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    "fg_edm_block_backward_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "fg_edm_run_block_backward": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "fg_edm_backward_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "fg_edm_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                c_size_t, c_void_p]),
    "fg_edm_forward_train": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                     c_size_t, c_void_p]),
    "fg_edm_backward_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                   c_int, c_void_p, c_size_t, c_void_p]),
    "fg_edm_backward_part": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                     c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "fg_edm2_create": (c_int, [POINTER(fg_edm2_config), POINTER(c_void_p)]),
    "fg_edm2_destroy": (None, [c_void_p]),
    "fg_edm2_num_params": (c_int, [c_void_p]),
    "fg_edm2_param_info": (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_int), POINTER(c_int64)]),
    "fg_edm2_bind_param": (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    "fg_edm2_pack_weights": (c_int, [c_void_p, c_void_p]),
    "fg_edm2_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "fg_edm2_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "fg_edm2_num_taps": (c_int, [c_void_p]),
    "fg_edm2_forward_taps": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p), c_int, c_int, c_void_p,
                                     c_size_t, c_void_p]),
    "fg_edm2_set_training": (c_int, [c_void_p, c_int]),
    "fg_edm2_sampler_run": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_double), c_int, c_int, c_int, c_void_p, c_uint64,
                                    c_void_p, c_int, c_void_p, c_size_t, c_int, c_void_p]),
    "fg_edm2_num_blocks": (c_int, [c_void_p]),
    "fg_edm2_block_info": (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_int), POINTER(c_int), POINTER(c_int),
                                   POINTER(c_int), POINTER(c_int)]),
    "fg_edm2_run_block": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                  c_size_t, c_void_p]),
    "fg_edm2_jvp_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "fg_edm2_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t,
                            c_void_p]),
    "fg_edm2_run_block_jvp": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "fg_dit_create": (c_int, [POINTER(fg_dit_config), POINTER(c_void_p)]),
    "fg_dit_destroy": (None, [c_void_p]),
    "fg_dit_num_params": (c_int, [c_void_p]),
    "fg_dit_param_info": (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_int), POINTER(c_int64)]),
    "fg_dit_bind_param": (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    "fg_dit_pack_weights": (c_int, [c_void_p, c_void_p]),
    "fg_dit_pack_group": (c_int, [c_void_p, c_char_p, c_char_p, c_void_p]),
    "fg_dit_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "fg_dit_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "fg_dit_forward_features": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int), POINTER(c_void_p),
                                        c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "fg_dit_jvp_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "fg_dit_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                           c_size_t, c_void_p]),
    "fg_op_dit_ln_modulate_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                          c_void_p]),
    "fg_op_dit_attention_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                        c_size_t, c_void_p]),
    "fg_op_dit_gelu_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "fg_dit_sampler_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "fg_dit_sampler_run": (c_int, [c_void_p, POINTER(fg_dit_sampler_config), c_void_p, c_void_p, c_void_p, POINTER(c_double), c_int, c_int, c_int,
                                   c_void_p, c_uint64, c_void_p, c_int, c_void_p, c_size_t, c_int, c_void_p]),
    "fg_wan_sampler_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "fg_wan_sampler_run": (c_int, [c_void_p, POINTER(fg_wan_sampler_config), c_void_p, POINTER(c_double), c_int, c_int, POINTER(c_int), c_void_p,
                                   c_uint64, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_int, c_void_p]),
    "fg_wan_guided_sampler_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int]),
    "fg_wan_guided_sampler_run": (c_int, [c_void_p, POINTER(fg_wan_guided_sampler_config), c_void_p, POINTER(c_double), POINTER(c_double), c_int,
                                          c_void_p, c_uint64, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_int, c_void_p]),
    "fg_op_guided_multistep": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p]),
    "fg_wan_select_cache_tag": (c_int, [c_void_p, c_int]),
    "fg_wan_create": (c_int, [POINTER(fg_wan_config), POINTER(c_void_p)]),
    "fg_wan_destroy": (None, [c_void_p]),
    "fg_wan_num_params": (c_int, [c_void_p]),
    "fg_wan_param_info": (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_int), POINTER(c_int64)]),
    "fg_wan_bind_param": (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    "fg_wan_pack_weights": (c_int, [c_void_p, c_void_p]),
    "fg_wan_pack_group": (c_int, [c_void_p, c_char_p, c_char_p, c_void_p]),
    "fg_wan_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "fg_wan_clear_caches": (c_int, [c_void_p, c_void_p]),
    "fg_wan_set_text": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "fg_wan_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                               c_void_p]),
    "fg_wan_forward_block_causal": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "fg_wan_forward_features": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_int),
                                        POINTER(fg_wan_block_taps), c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fg_wan_create_ex": (c_int, [POINTER(fg_wan_config), POINTER(fg_wan_ext_config), POINTER(c_void_p)]),
    "fg_wan_full_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "fg_wan_forward_full": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int), c_int, c_void_p,
                                    c_size_t, c_void_p]),
    "fg_wan_jvp_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "fg_wan_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                           POINTER(c_int), c_int, c_void_p, c_size_t, c_void_p]),
    "fg_op_wan_attention_jvp": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p,
                                        c_int, c_int64, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_wan_modulate_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                                       c_void_p]),
    "fg_op_wan_rms_rope_jvp": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fg_op_wan_gelu_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "fg_op_wan_final_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                    c_int, c_float, c_void_p]),
    "fg_wan_forward_full_features": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int), c_int,
                                             POINTER(c_int), POINTER(fg_wan_block_taps), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                             c_void_p]),
    "fg_wan_full_sampler_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "fg_wan_full_sampler_run": (c_int, [c_void_p, POINTER(fg_wan_sampler_config), c_void_p, POINTER(c_double), c_int, c_int, c_int, c_void_p,
                                        c_uint64, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_int, c_void_p]),
    "fg_wan_full_guided_sampler_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int]),
    "fg_wan_full_guided_sampler_run": (c_int, [c_void_p, POINTER(fg_wan_guided_sampler_config), c_void_p, POINTER(c_double), POINTER(c_double),
                                               c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_int, c_void_p]),
    "fg_wan_create_i2v": (c_int, [POINTER(fg_wan_config), POINTER(fg_wan_ext_config), POINTER(fg_wan_i2v_config), POINTER(c_void_p)]),
    "fg_wan_i2v_cond_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "fg_wan_set_i2v_cond": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "fg_wan_i2v_cond_read": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fg_wan_create_ti2v": (c_int, [POINTER(fg_wan_config), POINTER(fg_wan_ext_config), POINTER(fg_wan_ti2v_config), POINTER(c_void_p)]),
    "fg_wan_set_first_frame": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fg_wan_first_frame_read": (c_int, [c_void_p, c_void_p, c_void_p]),
    "fg_wan_create_vace": (c_int, [POINTER(fg_wan_config), POINTER(fg_wan_ext_config), POINTER(fg_wan_vace_config), POINTER(c_void_p)]),
    "fg_wan_set_vace_scale": (c_int, [c_void_p, POINTER(c_float), c_int, c_void_p]),
    "fg_wan_vace_context_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "fg_wan_set_vace_context": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "fg_wan_vace_context_read": (c_int, [c_void_p, c_void_p, c_void_p]),
    "fg_op_wan_vace_patch_embed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_wan_patch_embed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_wan_final": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int,
                                c_void_p]),
    "fg_op_wan_dual_cross_attention": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_int,
                                               c_int64, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_void_p]),
    "fg_disc_edm_num_params": (c_int, [c_int]),
    "fg_disc_edm_workspace_bytes": (c_size_t, [c_int, c_int]),
    "fg_disc_edm_run": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "fg_edm_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                           c_void_p, c_size_t, c_void_p]),
    "fg_edm_set_dropout": (c_int, [c_void_p, c_float, c_uint64]),
    "fg_op_gn_workspace_bytes": (c_size_t, [c_int, c_int]),
    "fg_op_gn_act": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_int,
                             c_float, ctypes.c_uint32, c_uint64, c_void_p, c_size_t, c_void_p]),
    "fg_op_gn_backward": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p,
                                  c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                  ctypes.c_uint32, c_uint64, c_void_p, c_size_t, c_void_p]),
    "fg_op_gn_jvp": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int,
                             c_float, ctypes.c_uint32, c_uint64, c_void_p, c_size_t, c_void_p]),
    "fg_op_attention_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "fg_op_attention_backward": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                         c_int, c_void_p, c_size_t, c_void_p]),
    "fg_op_attention_jvp": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                    c_void_p, c_size_t, c_void_p]),
    "fg_op_colsum": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_float, c_int, c_void_p]),
    "fg_op_batchsum_add": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fg_op_linear_backward": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int,
                                      c_void_p]),
    "fg_op_dgrad_weights": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_train_elementwise": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                        c_double, c_double, c_int, c_void_p]),
    "fg_op_edm_conv_pack_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "fg_op_edm_conv_pack": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_edm_conv_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    POINTER(fg_edm_conv_plan)]),
    "fg_op_edm_conv": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "fg_op_edm_gn_finalize": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int,
                                      c_int, c_void_p]),
    "fg_op_edm_gn_silu_pool": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fg_op_edm_attention": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "fg_op_edm_attn_merge_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "fg_op_edm_attention_merged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_void_p]),
    "fg_op_edm_head_pack_bytes": (c_size_t, [c_int, c_int, c_int]),
    "fg_op_edm_stem": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fg_op_edm_conv_in": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_edm_aux_head": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_void_p]),
    "fg_op_edm_aux_out": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                  c_void_p]),
    "fg_op_dropout_mask": (c_int, [c_void_p, c_int64, c_float, ctypes.c_uint32, c_uint64, c_void_p]),
    "fg_edm_set_augment": (c_int, [c_void_p, c_void_p]),
    "fg_edm_set_training": (c_int, [c_void_p, c_int]),
    "fg_op_images_to_u8": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "fg_op_randn": (c_int, [c_void_p, c_int64, c_uint64, c_uint64, c_void_p]),
    "fg_op_attention": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_attention_split": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_attention_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(fg_attention_plan)]),
    "fg_op_attention_ex": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_int64, c_int, c_int, c_int,
                                   c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "fg_op_dit_attention": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_size_t, c_int, c_void_p]),
    "fg_op_gemm_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_size_t, c_int, c_int, c_int, c_int, POINTER(fg_gemm_plan)]),
    "fg_op_gemm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                                c_int, c_void_p]),
    "fg_op_quant_rows_fp8": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "fg_op_gemm_fp8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                               c_int, c_void_p, c_void_p, c_void_p]),
    "fg_op_dit_ln_modulate_fp8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fg_op_gemm_x3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                              c_int, c_void_p]),
}

_lib = None


def lib():
    """Load (once) and return the library.  Raises if it has not been built: there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C fastgen_amd/csrc`).  fastgen_amd has no non-HIP fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def graph_stats():
    """(captures, launches) of `fg_graph_stats`: the hipGraphs the sampler entry points have instantiated and launched in this process.
    A call replayed its cached graph(s) if `captures` did not move across it."""
    c, n = c_uint64(), c_uint64()
    lib().fg_graph_stats(ctypes.byref(c), ctypes.byref(n))
    return c.value, n.value


class FastGenAMDError(RuntimeError):
    pass


def check(rc: int):
    if rc != 0:
        msg = lib().fg_last_error().decode("utf-8", "replace")
        raise FastGenAMDError(f"fastgen_amd error {rc}: {msg}")
