"""ctypes binding of liblavie_hip.so (C ABI: include/lavie_hip.h).

The library is built in-tree by `__graft_entry__.build()` / `make -C lavie_amd/csrc`.  There is no
fallback: if the shared object is missing or a call fails, a RuntimeError is raised."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LAVIE_HIP_LIB") or os.path.join(_HERE, "liblavie_hip.so")   # env override: A/B builds
ABI_VERSION = 8
FUSED_DEFAULT = 0x137    # lavie_debug_fused_mask: bits 0, 1, 2, 4, 5, 8 (include/lavie_hip.h)
MAX_LEVELS = 8
LORA_MAX_TERMS = 8       # LAVIE_LORA_MAX_TERMS: adapters blended in one merge = slots of the engine's registry
WINDOW_MAX_WINDOWS, WINDOW_MAX_LENGTH, WINDOW_MAX_COVER = 32, 64, 4      # LAVIE_WINDOW_MAX_*: limits of lavie_window_step

c_void_p, c_int, c_float, c_ll, c_char_p = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_char_p
c_float_p = C.c_void_p      # fp32 device pointers are passed as raw addresses
c_ull = C.c_ulonglong
NOISE_MAX_SEEDS = 16        # LAVIE_NOISE_MAX_SEEDS: latents of one seeded launch


class UNetConfigC(C.Structure):
    _fields_ = [
        ("struct_size", c_int),
        ("in_channels", c_int), ("out_channels", c_int), ("num_levels", c_int),
        ("block_out_channels", c_int * MAX_LEVELS), ("attn_levels", c_int * MAX_LEVELS),
        ("layers_per_block", c_int), ("heads", c_int), ("cross_attention_dim", c_int), ("norm_groups", c_int),
        ("norm_eps", c_float), ("rotary_dim", c_int), ("rel_buckets", c_int), ("rel_max_distance", c_int),
        ("sparse_causal_attn1", c_int), ("temporal_plain", c_int), ("ff_before_temporal", c_int),
        ("vsr_blocks", c_int), ("only_cross_attention", c_int * MAX_LEVELS),
        ("vsr_temporal_modules", c_int), ("num_class_embeds", c_int),
    ]


class LoraTermC(C.Structure):         # lavie_lora_term
    _fields_ = [("A", c_float_p), ("B", c_float_p), ("r", c_int), ("scale", c_float)]


class KnownRegionC(C.Structure):      # lavie_known_region
    _fields_ = [("struct_size", c_int), ("channels", c_int), ("inner", c_ll), ("known", c_float_p), ("mask", c_float_p),
                ("noise_known", c_float_p), ("a_next", c_float), ("s_next", c_float)]


class WindowStepArgsC(C.Structure):   # lavie_window_step_args
    _fields_ = [("struct_size", c_int), ("family", c_int), ("cfg", c_int), ("P", c_int), ("C", c_int), ("F", c_int), ("hw", c_ll),
                ("W", c_int), ("L", c_int), ("starts_host", C.POINTER(c_int)), ("profile_host", C.POINTER(c_float)),
                ("eps_host", C.POINTER(c_void_p)), ("model_in_host", C.POINTER(c_void_p)), ("x", c_float_p), ("aux", c_float_p),
                ("guidance", c_float), ("k_x", c_float), ("k_eps", c_float), ("c_x0", c_float), ("c_xt", c_float), ("c4", c_float),
                ("next_input_scale", c_float)]


class UnipcCoeffsC(C.Structure):      # lavie_unipc_coeffs (passed by value)
    _fields_ = [("struct_size", c_int), ("corr", c_int), ("guidance", c_float), ("k_x", c_float), ("k_eps", c_float), ("c_l", c_float),
                ("c_0", c_float), ("c_1", c_float), ("c_2", c_float), ("p_x", c_float), ("p_0", c_float), ("p_1", c_float),
                ("next_input_scale", c_float)]


class NoiseKeyC(C.Structure):         # lavie_noise_key
    _fields_ = [("struct_size", c_int), ("count", c_int), ("seeds_host", C.POINTER(c_ull)), ("per", c_ll), ("draw", c_ull)]


class DenoiseArgsC(C.Structure):        # lavie_denoise_args
    _fields_ = [("struct_size", c_int), ("x0_dtype", c_int), ("x0", c_void_p), ("a_host", C.POINTER(c_float)), ("s_host", C.POINTER(c_float)),
                ("offset_coef", c_float), ("offset_draw", c_ull), ("offset_hw", c_ll)]


class GuidanceTableArgsC(C.Structure):   # lavie_guidance_table_args
    _fields_ = [("struct_size", c_int), ("W", c_int), ("P", c_int), ("per", c_ll), ("eps_host", C.POINTER(c_void_p)),
                ("guidance_dev", c_float_p), ("guidance", c_float), ("rescale", c_float), ("partials", c_float_p),
                ("partials_floats", c_ll), ("table", c_float_p), ("moments", c_void_p)]


class FreqMixArgsC(C.Structure):      # lavie_freq_mix_args
    _fields_ = [("struct_size", c_int), ("images", c_int), ("F", c_int), ("H", c_int), ("W", c_int), ("x0", c_float_p), ("e0", c_float_p),
                ("z", c_float_p), ("filter", c_float_p), ("a", c_float), ("s", c_float), ("r", c_float), ("out", c_float_p),
                ("model_in", c_void_p), ("dup", c_int), ("dup_stride", c_ll), ("input_scale", c_float), ("workspace", c_void_p),
                ("workspace_bytes", c_ll)]


class OpStatisticsInfoC(C.Structure):   # lavie_op_statistics_info
    _fields_ = [("struct_size", c_int), ("M", c_int), ("N", c_int), ("splits", c_int), ("colstat_written", c_int), ("colstat_rows", c_int),
                ("colstat_span", c_int), ("nsets", c_int), ("set_blocks", c_int), ("colstat_contiguous", c_int),
                ("rowstat_written", c_int), ("rowstat_cols", c_int),
                ("rowstat_slots", c_int), ("colstat_blocks_stored", c_ll), ("colstat_floats", c_ll), ("rowstat_floats", c_ll)]


class GnProducerStatsC(C.Structure):    # lavie_gn_producer_stats
    _fields_ = [("struct_size", c_int), ("C", c_int), ("partials", c_float_p), ("partials_floats", c_ll), ("rows", c_int), ("nsets", c_int),
                ("set_blocks", c_int), ("span", c_int)]


class TextConfigC(C.Structure):        # lavie_text_config
    _fields_ = [("struct_size", c_int), ("vocab_size", c_int), ("hidden", c_int), ("intermediate", c_int), ("layers", c_int),
                ("heads", c_int), ("max_positions", c_int), ("act", c_int), ("eps", c_float)]


class VisionConfigC(C.Structure):      # lavie_vision_config
    _fields_ = [("struct_size", c_int), ("hidden", c_int), ("intermediate", c_int), ("layers", c_int), ("heads", c_int),
                ("image_size", c_int), ("patch_size", c_int), ("act", c_int), ("eps", c_float)]


class MapperConfigC(C.Structure):      # lavie_mapper_config
    _fields_ = [("struct_size", c_int), ("input_dim", c_int), ("output_dim", c_int), ("layers", c_int), ("heads", c_int),
                ("dim_feedforward", c_int), ("seq_in", c_int), ("seq_out", c_int), ("eps", c_float)]


class ClipPreprocessConfigC(C.Structure):   # lavie_clip_preprocess_config
    _fields_ = [("struct_size", c_int), ("size", c_int), ("crop", c_int), ("mean", c_float * 3), ("std", c_float * 3)]


# name -> (restype, argtypes); every symbol declared in include/lavie_hip.h
SIGNATURES = {
    "lavie_last_error": (c_char_p, []),
    "lavie_abi_version": (c_int, []),
    "lavie_linear_lnfold_f16": (c_int, [c_void_p, c_void_p, c_float_p, c_float_p, c_float_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "lavie_linear_lnfold_geglu_f16": (c_int, [c_void_p, c_void_p, c_float_p, c_float_p, c_float_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "lavie_linear_f16": (c_int, [c_void_p, c_int, c_void_p, c_float_p, c_float_p, c_int, c_int, c_void_p, c_int, c_void_p,
                                  c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "lavie_conv3x3_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_float_p,
                                   c_float_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                   c_void_p, c_void_p]),
    "lavie_conv3x3_down_f16": (c_int, [c_void_p, c_int, c_void_p, c_float_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p]),
    "lavie_pack_conv_edge_in_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "lavie_conv_edge_in_f16": (c_int, [c_void_p, c_int, c_void_p, c_float_p, c_float_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p]),
    "lavie_conv_edge_out_image_halfs": (c_ll, [c_int]),
    "lavie_pack_conv_edge_out_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "lavie_conv_edge_out_f16": (c_int, [c_void_p, c_void_p, c_float_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "lavie_pack_conv3x3_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "lavie_temporal_conv_f16": (c_int, [c_void_p, c_int, c_void_p, c_float_p, c_float_p, c_int, c_int, c_void_p, c_void_p, c_int,
                                         c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "lavie_pack_temporal_conv_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "lavie_pack_geglu_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_float_p, c_int, c_int, c_void_p]),
    "lavie_timestep_sinusoid_f32": (c_int, [c_float_p, c_float_p, c_int, c_int, c_void_p]),
    "lavie_gemv_f16": (c_int, [c_float_p, c_void_p, c_float_p, c_float_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "lavie_pack_conv_in_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "lavie_conv_in_f16": (c_int, [c_void_p, c_void_p, c_float_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "lavie_pack_conv_out_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "lavie_conv_out_f16": (c_int, [c_void_p, c_void_p, c_float_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "lavie_add_class_emb_silu_f32": (c_int, [c_float_p, c_void_p, C.POINTER(c_int), c_int, c_int, c_int, c_void_p]),
    "lavie_fill_relpos_bias_f32": (c_int, [c_void_p, c_void_p, c_float_p, c_int, c_int, c_int, c_void_p]),
    "lavie_ln_fold_f16": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_void_p, c_float_p, c_float_p, c_int, c_int, c_void_p]),
    "lavie_pack_geglu_vec_f32": (c_int, [c_float_p, c_float_p, c_int, c_void_p]),
    "lavie_copy_rows_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "lavie_f16_to_f32": (c_int, [c_void_p, c_void_p, c_float_p, c_ll, c_void_p]),
    "lavie_lora_merge_f16": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "lavie_lora_merge_multi_f16": (c_int, [c_void_p, C.POINTER(LoraTermC), c_int, c_void_p, c_int, c_int, c_void_p]),
    "lavie_freeu_workspace_bytes": (c_ll, [c_int, c_int, c_int, c_int]),
    "lavie_freeu_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "lavie_freq_mix_workspace_bytes": (c_ll, [c_int, c_int, c_int, c_int]),
    "lavie_freq_mix_f32": (c_int, [C.POINTER(FreqMixArgsC), c_void_p]),
    "lavie_geglu_mlp_image_bytes": (c_ll, [c_int]),
    "lavie_geglu_mlp_bias_floats": (c_ll, [c_int]),
    "lavie_pack_geglu_mlp_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_float_p, c_void_p]),
    "lavie_geglu_mlp_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                     c_float, c_void_p]),
    "lavie_temporal_block_image_bytes": (c_ll, [c_int, c_int, c_int, c_int]),
    "lavie_pack_temporal_block_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "lavie_temporal_block_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_float_p, c_float_p,
                                          c_float_p, c_float_p, c_float_p, c_float_p, c_int, c_float, c_float, c_void_p]),
    "lavie_cross_block_image_bytes": (c_ll, [c_int, c_int]),
    "lavie_pack_cross_block_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "lavie_bind_cross_block_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "lavie_cross_block_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_float_p, c_float_p,
                                       c_float_p, c_float_p, c_int, c_float, c_float, c_void_p]),
    "lavie_cross_block_long_image_bytes": (c_ll, [c_int, c_int]),
    "lavie_pack_cross_block_long_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "lavie_bind_cross_block_long_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "lavie_cross_block_long_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_float_p, c_float_p,
                                            c_float_p, c_float_p, c_int, c_float, c_float, c_void_p]),
    "lavie_pack_conv3x3_parity_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "lavie_upsample_conv3x3_supported": (c_int, [c_int, c_int, c_int, c_int]),
    "lavie_upsample_conv3x3_f16": (c_int, [c_void_p, c_void_p, c_float_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "lavie_proj_qkv_image_bytes": (c_ll, [c_int]),
    "lavie_pack_proj_qkv_f16": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "lavie_group_norm_affine_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float_p, c_float_p, c_float, c_float_p, c_float_p, c_void_p]),
    "lavie_proj_qkv_f16": (c_int, [c_void_p, c_float_p, c_int, c_void_p, c_float_p, c_float_p, c_float_p, c_float, c_void_p, c_void_p,
                                    c_int, c_int, c_void_p]),
    "lavie_group_norm_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_float_p, c_float_p, c_float,
                                      c_int, c_float_p, c_void_p, c_void_p]),
    "lavie_group_norm_ws_floats": (c_ll, [c_int, c_int]),
    "lavie_layer_norm_f16": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "lavie_attention_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                     c_int, c_int, c_int, c_float, c_void_p]),
    "lavie_sparse_causal_attention_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
                                                   c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "lavie_temporal_attention_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float_p,
                                              c_float_p, c_float_p, c_int, c_float, c_void_p]),
    "lavie_relpos_buckets": (c_int, [c_int, c_int, c_int, C.POINTER(c_int)]),
    "lavie_cfg_ddpm_step": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float,
                                     c_float, c_float, c_void_p]),
    "lavie_latents_to_model_input": (c_int, [c_float_p, c_void_p, c_ll, c_void_p]),
    "lavie_cfg_sampler_step": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float,
                                        c_float, c_float, c_float, c_void_p]),
    "lavie_latents_to_scaled_model_input": (c_int, [c_float_p, c_void_p, c_ll, c_float, c_void_p]),
    "lavie_sampler_step": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float, c_float,
                                    c_float, c_void_p]),
    "lavie_latents_to_scaled_model_input1": (c_int, [c_float_p, c_void_p, c_ll, c_float, c_void_p]),
    "lavie_cfg_multistep_step": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float,
                                          c_float, c_float, c_float, c_void_p]),
    "lavie_multistep_step": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float, c_float,
                                      c_float, c_void_p]),
    "lavie_cfg_sampler_step_known": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float,
                                              c_float, c_float, c_float, c_void_p, C.POINTER(KnownRegionC)]),
    "lavie_sampler_step_known": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float, c_float,
                                          c_float, c_void_p, C.POINTER(KnownRegionC)]),
    "lavie_cfg_multistep_step_known": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float,
                                                c_float, c_float, c_float, c_void_p, C.POINTER(KnownRegionC)]),
    "lavie_multistep_step_known": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float,
                                            c_float, c_float, c_void_p, C.POINTER(KnownRegionC)]),
    "lavie_known_blend_f32": (c_int, [c_float_p, c_void_p, c_int, c_ll, c_float, c_void_p, C.POINTER(KnownRegionC)]),
    "lavie_window_step": (c_int, [C.POINTER(WindowStepArgsC), c_void_p]),
    "lavie_guidance_partials_floats": (c_ll, [c_int, c_ll]),
    "lavie_guidance_table": (c_int, [C.POINTER(GuidanceTableArgsC), c_void_p]),
    "lavie_cfg_sampler_step_scaled": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float_p, c_ll, c_float, c_float, c_float,
                                               c_float, c_float, c_float, c_void_p]),
    "lavie_cfg_multistep_step_scaled": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float_p, c_ll, c_float, c_float,
                                                 c_float, c_float, c_float, c_float, c_void_p]),
    "lavie_cfg_sampler_step_known_scaled": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float_p, c_float, c_float, c_float,
                                                     c_float, c_float, c_float, c_void_p, C.POINTER(KnownRegionC)]),
    "lavie_cfg_multistep_step_known_scaled": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float_p, c_float, c_float,
                                                       c_float, c_float, c_float, c_float, c_void_p, C.POINTER(KnownRegionC)]),
    "lavie_window_step_scaled": (c_int, [C.POINTER(WindowStepArgsC), c_float_p, c_void_p]),
    "lavie_cfg_pag_sampler_step": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float, c_float,
                                            c_float, c_float, c_float, c_void_p]),
    "lavie_pag_sampler_step": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float, c_float,
                                        c_float, c_float, c_void_p]),
    "lavie_unipc_step": (c_int, [c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_void_p, c_ll, UnipcCoeffsC, c_void_p]),
    "lavie_cfg_unipc_step": (c_int, [c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_void_p, c_ll, UnipcCoeffsC, c_void_p]),
    "lavie_cfg_unipc_step_scaled": (c_int, [c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_void_p, c_ll, c_float_p, c_ll,
                                            UnipcCoeffsC, c_void_p]),
    "lavie_cfg_pag_multistep_step": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float, c_float,
                                              c_float, c_float, c_float, c_void_p]),
    "lavie_pag_multistep_step": (c_int, [c_void_p, c_float_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float, c_float,
                                          c_float, c_float, c_void_p]),
    "lavie_debug_force_tile": (c_int, [c_int]),
    "lavie_debug_force_splits": (c_int, [c_int]),
    "lavie_debug_fused_mask": (c_int, [c_int]),
    "lavie_debug_gn_producer_count": (c_ll, []),
    "lavie_debug_op_statistics": (c_int, [c_float_p, c_ll, c_float_p, c_ll]),
    "lavie_debug_op_statistics_plan": (c_int, [c_int, c_int]),
    "lavie_debug_op_statistics_last": (c_int, [C.POINTER(OpStatisticsInfoC)]),
    "lavie_group_norm_stats_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_float_p, c_float_p, c_float,
                                            c_int, c_float_p, c_void_p, C.POINTER(GnProducerStatsC), C.POINTER(GnProducerStatsC), c_void_p]),
    "lavie_rowstat_finalize_f32": (c_int, [c_float_p, c_int, c_int, c_int, c_float, c_float_p, c_void_p]),
    "lavie_debug_temporal_budget": (c_int, [c_int]),
    "lavie_debug_rowfuse_grid": (c_int, [c_int]),
    "lavie_profile_begin": (c_int, [C.c_uint, c_int]),
    "lavie_profile_end": (c_int, [c_void_p, C.POINTER(c_ll), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_double)]),
    "lavie_unet_config_size": (c_int, []),
    "lavie_unet_create": (c_int, [C.POINTER(UNetConfigC), C.POINTER(c_void_p)]),
    "lavie_unet_destroy": (c_int, [c_void_p]),
    "lavie_unet_num_params": (c_int, [c_void_p]),
    "lavie_unet_param_info": (c_int, [c_void_p, c_int, C.POINTER(c_char_p), C.POINTER(c_ll)]),
    "lavie_unet_set_param": (c_int, [c_void_p, c_char_p, c_void_p, c_ll]),
    "lavie_unet_finalize": (c_int, [c_void_p, c_void_p]),
    "lavie_unet_prepare": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "lavie_unet_cache_context": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "lavie_unet_set_ln_fold": (c_int, [c_void_p, c_int]),
    "lavie_unet_lora_set": (c_int, [c_void_p, c_char_p, c_void_p, c_float_p, c_float_p, c_int, c_float, c_void_p]),
    "lavie_unet_lora_clear": (c_int, [c_void_p, c_char_p, c_void_p]),
    "lavie_unet_lora_set_scale": (c_int, [c_void_p, c_float]),
    "lavie_unet_lora_apply": (c_int, [c_void_p, c_void_p]),
    "lavie_unet_lora_set_slot": (c_int, [c_void_p, c_int, c_char_p, c_void_p, c_float_p, c_float_p, c_int, c_float, c_void_p]),
    "lavie_unet_lora_clear_slot": (c_int, [c_void_p, c_int, c_char_p, c_void_p]),
    "lavie_unet_lora_set_slot_weight": (c_int, [c_void_p, c_int, c_float]),
    "lavie_unet_set_cfg_shared_input": (c_int, [c_void_p, c_int]),
    "lavie_unet_set_freeu": (c_int, [c_void_p, c_float, c_float, c_float, c_float]),
    "lavie_unet_set_pag": (c_int, [c_void_p, C.POINTER(c_char_p), c_int, c_int]),
    "lavie_unet_weight_bytes": (c_ll, [c_void_p]),
    "lavie_unet_workspace_bytes": (c_ll, [c_void_p]),
    "lavie_unet_forward": (c_int, [c_void_p, c_void_p, c_float_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                    c_void_p]),
    "lavie_unet_forward_graph": (c_int, [c_void_p, c_void_p, c_float_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                          c_void_p]),
    "lavie_unet_set_layer_cache": (c_int, [c_void_p, c_int]),
    "lavie_unet_layer_cache_bytes": (c_ll, [c_void_p]),
    "lavie_unet_forward_cached": (c_int, [c_void_p, c_void_p, c_float_p, c_void_p, C.POINTER(c_int), c_void_p, c_int, c_int,
                                          c_int, c_int, c_int, c_int, c_void_p]),
    "lavie_unet_forward_labels": (c_int, [c_void_p, c_void_p, c_float_p, c_void_p, C.POINTER(c_int), c_void_p, c_int, c_int,
                                           c_int, c_int, c_int, c_void_p]),
    "lavie_unet_resnet_forward": (c_int, [c_void_p, c_char_p, c_void_p, c_int, c_void_p, c_int, c_float_p, c_void_p, c_int,
                                           c_int, c_int, c_int, c_void_p]),
    "lavie_unet_transformer_forward": (c_int, [c_void_p, c_char_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                                c_void_p]),
    "lavie_causal_attention_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "lavie_token_embed_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "lavie_act_f16": (c_int, [c_void_p, c_ll, c_int, c_void_p]),
    "lavie_text_config_size": (c_int, []),
    "lavie_text_create": (c_int, [C.POINTER(TextConfigC), C.POINTER(c_void_p)]),
    "lavie_text_destroy": (c_int, [c_void_p]),
    "lavie_text_num_params": (c_int, [c_void_p]),
    "lavie_text_param_info": (c_int, [c_void_p, c_int, C.POINTER(c_char_p), C.POINTER(c_ll)]),
    "lavie_text_set_param": (c_int, [c_void_p, c_char_p, c_void_p, c_ll]),
    "lavie_text_finalize": (c_int, [c_void_p, c_void_p]),
    "lavie_text_workspace_bytes": (c_ll, [c_void_p, c_int, c_int]),
    "lavie_text_encode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "lavie_short_attention_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                           c_int, c_float, c_void_p]),
    "lavie_patch_embed_k": (c_int, [c_int]),
    "lavie_patch_embed_workspace_bytes": (c_ll, [c_int, c_int, c_int]),
    "lavie_pack_patch_embed_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "lavie_patch_embed_f16": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                       c_void_p]),
    "lavie_relu_f16": (c_int, [c_void_p, c_ll, c_void_p]),
    "lavie_vision_config_size": (c_int, []),
    "lavie_vision_create": (c_int, [C.POINTER(VisionConfigC), C.POINTER(c_void_p)]),
    "lavie_vision_destroy": (c_int, [c_void_p]),
    "lavie_vision_num_params": (c_int, [c_void_p]),
    "lavie_vision_param_info": (c_int, [c_void_p, c_int, C.POINTER(c_char_p), C.POINTER(c_ll)]),
    "lavie_vision_set_param": (c_int, [c_void_p, c_char_p, c_void_p, c_ll]),
    "lavie_vision_finalize": (c_int, [c_void_p, c_void_p]),
    "lavie_vision_workspace_bytes": (c_ll, [c_void_p, c_int]),
    "lavie_vision_encode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "lavie_mapper_config_size": (c_int, []),
    "lavie_mapper_create": (c_int, [C.POINTER(MapperConfigC), C.POINTER(c_void_p)]),
    "lavie_mapper_destroy": (c_int, [c_void_p]),
    "lavie_mapper_num_params": (c_int, [c_void_p]),
    "lavie_mapper_param_info": (c_int, [c_void_p, c_int, C.POINTER(c_char_p), C.POINTER(c_ll)]),
    "lavie_mapper_set_param": (c_int, [c_void_p, c_char_p, c_void_p, c_ll]),
    "lavie_mapper_finalize": (c_int, [c_void_p, c_void_p]),
    "lavie_mapper_workspace_bytes": (c_ll, [c_void_p, c_int]),
    "lavie_mapper_encode": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "lavie_pinned_linear_f16": (c_int, [c_void_p, c_int, c_void_p, c_float_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "lavie_add_rows_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "lavie_philox4x32_host": (c_int, [C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "lavie_philox_normal_f32": (c_int, [c_float_p, C.POINTER(c_ull), c_int, c_ll, c_ll, c_ull, c_void_p]),
    "lavie_sampler_step_seeded": (c_int, [c_void_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float, c_float, c_float,
                                           c_void_p, C.POINTER(NoiseKeyC)]),
    "lavie_cfg_sampler_step_seeded": (c_int, [c_void_p, c_float_p, c_void_p, c_ll, c_float, c_float, c_float, c_float, c_float, c_float,
                                               c_float, c_void_p, C.POINTER(NoiseKeyC)]),
    "lavie_window_step_seeded": (c_int, [C.POINTER(WindowStepArgsC), C.POINTER(NoiseKeyC), c_void_p]),
    "lavie_debug_noise_key_refusal": (c_int, [c_int]),
    "lavie_noisy_latents_seeded": (c_int, [C.POINTER(DenoiseArgsC), C.POINTER(NoiseKeyC), c_void_p, c_void_p]),
    "lavie_denoising_loss_workspace_floats": (c_ll, [c_int, c_ll]),
    "lavie_denoising_loss_f32": (c_int, [C.POINTER(DenoiseArgsC), C.POINTER(NoiseKeyC), c_void_p, c_int, c_float_p, c_float_p, c_ll, c_void_p]),
    "lavie_clip_resample_table_host": (c_int, [c_int, c_int, C.POINTER(c_int), C.POINTER(c_int), C.POINTER(c_int)]),
    "lavie_clip_preprocess_workspace_bytes": (c_ll, [c_int, c_int, c_int, c_int, c_int]),
    "lavie_clip_preprocess_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_ll, c_ll, c_void_p, c_int, C.POINTER(ClipPreprocessConfigC), c_void_p,
                                         c_ll, c_void_p]),
    "lavie_clip_embed_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_float_p, c_float_p, c_float, c_void_p, c_int,
                                     c_int, c_float_p, c_void_p]),
    "lavie_clip_similarity_f32": (c_int, [c_float_p, c_float_p, c_float_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "lavie_conv3d_packed_halfs": (c_ll, [c_int, c_int, c_int, c_int, c_int]),
    "lavie_conv3d_pack": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "lavie_conv3d_fold_pack_f32": (c_int, [c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, C.c_double, c_void_p, c_float_p, c_int, c_int,
                                           c_int, c_int, c_int, c_void_p]),
    "lavie_conv3d_f16": (c_int, [c_void_p, c_void_p, c_float_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                 c_int, c_void_p]),
    "lavie_conv3d_stem_f16": (c_int, [c_void_p, c_int, c_ll, c_ll, c_ll, c_void_p, c_float_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                      c_void_p]),
    "lavie_mean_rows_f32": (c_int, [c_void_p, c_float_p, c_int, c_int, c_int, c_void_p]),
    "lavie_r3d_create": (c_int, [C.POINTER(c_void_p)]),
    "lavie_r3d_destroy": (c_int, [c_void_p]),
    "lavie_r3d_num_params": (c_int, [c_void_p]),
    "lavie_r3d_param_info": (c_int, [c_void_p, c_int, C.POINTER(c_char_p), C.POINTER(c_ll)]),
    "lavie_r3d_set_param": (c_int, [c_void_p, c_char_p, c_void_p, c_ll]),
    "lavie_r3d_finalize": (c_int, [c_void_p, c_void_p]),
    "lavie_r3d_workspace_bytes": (c_ll, [c_void_p, c_int, c_int, c_int, c_int]),
    "lavie_r3d_features": (c_int, [c_void_p, c_void_p, c_int, c_ll, c_ll, c_ll, c_int, c_int, c_int, c_int, c_float_p, c_void_p, c_ll,
                                   c_void_p]),
    "lavie_video_resample_table_host": (c_int, [c_int, c_int, C.POINTER(c_int), C.POINTER(c_int), C.POINTER(c_int)]),
    "lavie_video_preprocess_workspace_bytes": (c_ll, [c_int, c_int, c_int, c_int, c_int]),
    "lavie_video_preprocess_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_ll, c_ll, c_void_p, c_int, c_int, c_int, C.POINTER(c_float),
                                          C.POINTER(c_float), c_void_p, c_ll, c_void_p]),
}

_lib = None


def load():
    """Returns the bound CDLL; raises RuntimeError if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C lavie_amd/csrc).  lavie_amd has no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so and the library links the same SONAME.
    # Whichever copy is loaded first serves both; if this library came first (its /opt/rocm copy) and torch later
    # loaded its own, the two runtimes would not see each other's device (hipMalloc: "no ROCm-capable device").
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)      # AttributeError here = header/library mismatch
        except AttributeError:
            if os.environ.get("LAVIE_HIP_LIB"):
                continue                  # A/B run against an older build: tolerate missing debug symbols
            raise
        fn.restype = res
        fn.argtypes = args
    if lib.lavie_abi_version() != ABI_VERSION and not os.environ.get("LAVIE_HIP_LIB"):
        raise RuntimeError(f"liblavie_hip.so ABI {lib.lavie_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str = "lavie call"):
    if rc != 0:
        msg = load().lavie_last_error()
        raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else 'unknown error'}")
