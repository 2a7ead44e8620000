"""ctypes binding of libdmhomo_hip.so (C ABI declared in include/dmhomo_hip.h).

The product path has no CPU or PyTorch-eager fallback: if the shared library is
missing or a symbol cannot be resolved, importing / calling fails loudly.
Tensors cross the boundary as raw device pointers (``tensor.data_ptr()``) plus
sizes; the HIP stream is torch's current stream.
"""
import contextlib
import ctypes as C
import gc
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DMH_LIB_PATH: development knob for A/B runs of two builds in one process environment (same GPU, same clocks)
LIB_PATH = os.environ.get('DMH_LIB_PATH') or os.path.join(_HERE, 'libdmhomo_hip.so')

c_f32p = C.c_void_p
c_i64 = C.c_int64
c_int = C.c_int
c_float = C.c_float


ABI_VERSION = 500          # include/dmhomo_hip.h: DMH_ABI_VERSION


class DmhConv(C.Structure):
    _fields_ = [('struct_size', C.c_uint64)] + \
               [(n, C.c_void_p) for n in ('src0', 'src1', 'wpack', 'bias', 'in_coef', 'res', 'res_coef', 'out',
                                          'stats')] + \
               [(n, C.c_int32) for n in ('B', 'Hin', 'Win', 'C0', 'C1', 'Cout', 'KH', 'KW', 'stride', 'upsample2')] + \
               [('in_bound', C.c_void_p), ('in_bound_n', C.c_int32), ('fin_n', C.c_int32), ('fin_w', C.c_void_p),
                ('fin_b', C.c_void_p), ('fin_out', C.c_void_p), ('pix_stats', C.c_void_p), ('pix_eps', C.c_float),
                ('rows', C.c_void_p)]


class DmhPackJob(C.Structure):
    _fields_ = [('src', C.c_void_p), ('ws', C.c_void_p), ('wpack', C.c_void_p), ('Cout', C.c_int32), ('C0', C.c_int32),
                ('C1', C.c_int32), ('KH', C.c_int32), ('transposed', C.c_int32)]


class DmhStep(C.Structure):
    _fields_ = [('objective', C.c_int32), ('clip', C.c_int32), ('mode', C.c_int32), ('cond_scale', C.c_float),
                ('sqrt_recip_ac', C.c_float), ('sqrt_recipm1_ac', C.c_float), ('sqrt_ac', C.c_float),
                ('sqrt_1m_ac', C.c_float), ('c0', C.c_float), ('c1', C.c_float), ('c2', C.c_float)]


# name -> (restype, argtypes); every symbol include/dmhomo_hip.h declares
SIGNATURES = {
    'dmh_last_error': (C.c_char_p, []),
    'dmh_version': (c_int, []),
    'dmh_ws_standardize': (c_int, [c_f32p, c_f32p, c_int, c_int, c_float, C.c_void_p]),
    'dmh_conv_pack_floats': (c_i64, [c_int, c_int, c_int, c_int, c_int]),
    'dmh_pack_conv_weight': (c_int, [c_f32p, c_f32p, c_int, c_int, c_int, c_int, c_int, C.c_void_p]),
    'dmh_pack_conv_weights_multi': (c_int, [C.c_void_p, c_int, c_float, C.c_void_p]),
    'dmh_conv_up2_pack_floats': (c_i64, [c_int, c_int]),
    'dmh_pack_conv_weight_up2': (c_int, [c_f32p, c_f32p, c_int, c_int, C.c_void_p]),
    'dmh_conv_tiles': (c_int, [c_int, c_int, c_int, c_int]),
    'dmh_conv2d': (c_int, [C.POINTER(DmhConv), C.c_void_p]),
    'dmh_rows_from_keep': (c_int, [C.c_void_p, c_int, c_int, C.c_void_p, C.c_void_p]),
    'dmh_gn_finalize': (c_int, [c_f32p, c_int, c_f32p, c_f32p, c_f32p, c_i64, c_f32p, c_int, c_int, c_int, c_int,
                                c_float, C.c_void_p, C.c_void_p]),
    'dmh_gn_finalize_bound': (c_int, [c_f32p, c_int, c_f32p, c_f32p, c_f32p, c_i64, c_f32p, c_f32p, c_int, c_int, c_int,
                                      c_int, c_float, C.c_void_p, C.c_void_p]),
    'dmh_gn_silu_residual': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int, C.c_void_p, C.c_void_p]),
    'dmh_gn_silu_residual_stats': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int, c_float, C.c_void_p,
                                           C.c_void_p]),
    'dmh_chan_layernorm': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_i64, c_int, c_float, C.c_void_p, c_i64, C.c_void_p]),
    'dmh_linattn_splits': (c_int, [c_int]),
    'dmh_linattn_partial_floats': (c_i64, [c_int, c_int]),
    'dmh_linattn_context': (c_int, [c_f32p, c_f32p, c_int, c_int, C.c_void_p, C.c_void_p]),
    'dmh_linattn_merge': (c_int, [c_f32p, c_f32p, c_int, c_int, C.c_void_p, C.c_void_p]),
    'dmh_linattn_apply': (c_int, [c_f32p, c_f32p, c_f32p, c_int, c_int, c_float, C.c_void_p, C.c_void_p]),
    'dmh_conv_wgrad_workspace_floats': (c_i64, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'dmh_conv_wgrad': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int, c_int, c_int,
                               c_int, c_int, c_int, C.c_void_p]),
    'dmh_conv_unshuffle_wgrad_workspace_floats': (c_i64, [c_int, c_int, c_int, c_int, c_int]),
    'dmh_conv_unshuffle_wgrad': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int, c_int, c_int, C.c_void_p]),
    'dmh_s2d_shift': (c_int, [c_f32p, c_f32p, c_int, c_int, c_int, c_int, C.c_void_p]),
    'dmh_d2s': (c_int, [c_f32p, c_f32p, c_int, c_int, c_int, c_int, C.c_void_p]),
    'dmh_sumpool2': (c_int, [c_f32p, c_f32p, c_int, c_int, c_int, c_int, C.c_void_p]),
    'dmh_gn_finalize_train': (c_int, [c_f32p, c_int, c_f32p, c_f32p, c_f32p, c_i64, c_f32p, c_f32p, c_int, c_int, c_int,
                                      c_int, c_float, C.c_void_p]),
    'dmh_gn_bwd_chunks': (c_int, [c_int]),
    'dmh_gn_silu_backward': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i64, c_f32p, c_f32p, c_f32p,
                                     c_f32p, c_int, c_int, c_int, c_int, C.c_void_p]),
    'dmh_sum_over_batch': (c_int, [c_f32p, c_f32p, c_int, c_i64, C.c_void_p]),
    'dmh_ws_backward': (c_int, [c_f32p, c_f32p, c_f32p, c_int, c_int, c_float, C.c_void_p]),
    'dmh_lnb_blocks': (c_int, []),
    'dmh_chan_layernorm_backward': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i64, c_int, c_float, C.c_void_p]),
    'dmh_linattn_merge_ms': (c_int, [c_f32p, c_f32p, c_f32p, c_int, c_int, C.c_void_p]),
    'dmh_linattn_bwd_workspace_floats': (c_i64, [c_int, c_int]),
    'dmh_linattn_backward': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_float, C.c_void_p]),
    'dmh_bgemm': (c_int, [c_f32p, C.POINTER(c_i64), c_f32p, C.POINTER(c_i64), c_f32p, C.POINTER(c_i64), c_int, c_int, c_int,
                          c_int, c_int, c_float, C.c_void_p]),
    'dmh_softmax_rows': (c_int, [c_f32p, c_f32p, c_i64, c_int, C.c_void_p]),
    'dmh_softmax_rows_backward': (c_int, [c_f32p, c_f32p, c_i64, c_int, C.c_void_p]),
    'dmh_act': (c_int, [c_f32p, c_f32p, c_f32p, c_i64, c_int, C.c_void_p]),
    'dmh_class_embed_backward': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int, C.c_void_p]),
    'dmh_loss_backward_ddp': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_i64, c_int, c_float, C.c_void_p]),
    'dmh_loss_backward': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int, c_int,
                                  C.c_void_p]),
    'dmh_sumsq_blocks': (c_int, []),
    'dmh_sumsq': (c_int, [c_f32p, c_i64, c_f32p, C.c_void_p]),
    'dmh_gradnorm_finalize': (c_int, [c_f32p, c_int, c_float, c_f32p, C.c_void_p]),
    'dmh_adam': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i64, c_float, c_float, c_float, c_float, c_int,
                         C.c_void_p]),
    'dmh_ema': (c_int, [c_f32p, c_f32p, c_i64, c_float, C.c_void_p]),
    'dmh_multi_blocks': (c_i64, [C.c_void_p, c_int]),
    'dmh_sumsq_multi': (c_int, [C.c_void_p, C.c_void_p, c_int, c_f32p, C.c_void_p]),
    'dmh_adam_multi': (c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_int, c_f32p, c_float, c_float,
                               c_float, c_float, c_int, C.c_void_p]),
    'dmh_resize_bilinear_u8': (c_int, [C.c_void_p, c_f32p, c_int, c_int, c_int, c_int, c_int, c_int, c_i64, c_float,
                                       C.c_void_p]),
    'dmh_mask_open_nearest': (c_int, [c_f32p, c_f32p, c_int, c_int, c_int, c_int, c_int, c_i64, C.c_void_p]),
    'dmh_pixel_stats': (c_int, [c_f32p, c_f32p, c_i64, c_int, c_float, C.c_void_p, c_i64, C.c_void_p]),
    'dmh_linattn_fused_pack_floats': (c_i64, [c_int]),
    'dmh_linattn_fused_pack': (c_int, [c_f32p, c_f32p, c_int, C.c_void_p]),
    'dmh_linattn_fused_splits': (c_int, [c_int, c_int]),
    'dmh_linattn_fused_context': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int, C.c_void_p, C.c_void_p]),
    'dmh_linattn_out_pack_floats': (c_i64, []),
    'dmh_linattn_out_pack': (c_int, [c_f32p, c_f32p, C.c_void_p]),
    'dmh_linattn_fused_apply_out': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int,
                                            c_int, c_int, c_float, c_float, C.c_void_p, C.c_void_p]),
    'dmh_linattn_merge_n': (c_int, [c_f32p, c_f32p, c_int, c_int, c_int, C.c_void_p, C.c_void_p]),
    'dmh_linattn_fused_apply': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int, c_float,
                                        C.c_void_p, C.c_void_p]),
    'dmh_attention': (c_int, [c_f32p, c_f32p, c_int, c_int, c_float, C.c_void_p, C.c_void_p]),
    'dmh_sinusoidal_embed': (c_int, [C.c_void_p, c_f32p, c_f32p, c_int, c_int, C.c_void_p]),
    'dmh_fourier_embed': (c_int, [C.c_void_p, c_f32p, c_f32p, c_int, c_int, C.c_void_p]),
    'dmh_class_embed': (c_int, [C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int, C.c_void_p]),
    'dmh_linear': (c_int, [c_f32p, c_i64, c_f32p, c_f32p, c_f32p, c_i64, c_int, c_int, c_int, c_int, c_int,
                           C.c_void_p]),
    'dmh_ss_gather': (c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p, C.c_void_p, c_int, c_f32p, c_int, c_int, c_int,
                              C.c_void_p]),
    'dmh_assemble_input': (c_int, [c_f32p, c_int, c_f32p, c_int, c_f32p, c_f32p, c_int, c_int, c_int, c_int,
                                   C.c_void_p]),
    'dmh_final_conv_nchw': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int, c_int, C.c_void_p]),
    'dmh_sampler_step': (c_int, [C.POINTER(DmhStep), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i64,
                                 C.c_void_p, c_i64, C.c_void_p]),
    'dmh_sampler_step_dev': (c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i64, C.c_void_p,
                                     c_i64, C.c_void_p]),
    'dmh_sampler_seek': (c_int, [C.c_void_p, c_int, C.c_void_p, C.c_void_p, c_int, C.c_void_p, C.c_void_p, c_int,
                                 C.c_void_p]),
    'dmh_sampler_step_ddp_dev': (c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p,
                                         c_f32p, c_f32p, c_int, c_int, c_int, c_int, c_int, C.c_void_p]),
    'dmh_sampler_step_ms': (c_int, [C.POINTER(DmhStep), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i64, C.c_void_p,
                                    c_i64, C.c_void_p]),
    'dmh_sampler_step_ms_dev': (c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i64, C.c_void_p, c_i64,
                                        C.c_void_p]),
    'dmh_sampler_step_ddp_ms_dev': (c_int, [C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int,
                                            c_int, c_int, C.c_void_p]),
    'dmh_row_quantile_abs': (c_int, [c_f32p, c_f32p, c_int, c_i64, c_i64, c_float, c_float, C.c_void_p]),
    'dmh_sampler_threshold': (c_int, [C.POINTER(DmhStep), c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_int, c_i64,
                                      c_i64, c_float, C.c_void_p]),
    'dmh_sampler_threshold_dev': (c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_int, c_i64, c_i64,
                                          c_float, C.c_void_p]),
    'dmh_sampler_step_thr': (c_int, [C.POINTER(DmhStep), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i64,
                                     C.c_void_p, c_i64, C.c_void_p]),
    'dmh_sampler_step_thr_dev': (c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i64,
                                         C.c_void_p, c_i64, C.c_void_p]),
    'dmh_guidance_splits': (c_int, [c_int, c_i64]),
    'dmh_guidance_factor': (c_int, [C.POINTER(DmhStep), c_f32p, c_f32p, C.c_void_p, c_float, C.c_void_p, c_f32p, c_int, c_i64,
                                    C.c_void_p]),
    'dmh_guidance_factor_dev': (c_int, [C.c_void_p, c_f32p, c_f32p, C.c_void_p, c_float, C.c_void_p, c_f32p, c_int, c_i64,
                                        C.c_void_p]),
    'dmh_sampler_threshold_gr': (c_int, [C.POINTER(DmhStep), c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_int,
                                         c_i64, c_i64, c_float, C.c_void_p]),
    'dmh_sampler_threshold_gr_dev': (c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_int, c_i64,
                                             c_i64, c_float, C.c_void_p]),
    'dmh_sampler_step_gr': (c_int, [C.POINTER(DmhStep), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                    c_i64, C.c_void_p, c_i64, C.c_void_p]),
    'dmh_sampler_step_gr_dev': (c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                        c_i64, C.c_void_p, c_i64, C.c_void_p]),
    'dmh_rows_gated': (c_int, [C.c_void_p, c_int, c_int, C.c_void_p, C.c_void_p, c_int, c_int, C.c_void_p, C.c_void_p]),
    'dmh_guidance_gate': (c_int, [C.c_void_p, C.c_void_p, c_int, c_f32p, c_f32p, c_i64, C.c_void_p]),
    'dmh_apg_splits': (c_int, [c_int, c_i64]),
    'dmh_apg_coef': (c_int, [C.POINTER(DmhStep), c_f32p, c_f32p, C.c_void_p, c_float, c_float, c_float, c_f32p, C.c_void_p, c_f32p,
                             c_int, c_i64, C.c_void_p]),
    'dmh_apg_coef_dev': (c_int, [C.c_void_p, c_f32p, c_f32p, C.c_void_p, c_float, c_float, c_float, c_f32p, C.c_void_p, c_f32p,
                                 c_int, c_i64, C.c_void_p]),
    'dmh_apg_apply': (c_int, [c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_int, c_i64, C.c_void_p]),
    'dmh_photo_acc_words': (c_i64, [c_int, c_int, c_int]),
    'dmh_photo_energy_splits': (c_int, [c_int, c_int, c_int]),
    'dmh_photo_weights': (c_int, [c_f32p, c_f32p, C.c_void_p, c_f32p, c_int, c_int, c_int, C.c_void_p]),
    'dmh_photo_guide': (c_int, [C.POINTER(DmhStep), c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_float, C.c_void_p,
                                c_f32p, c_int, c_int, c_int, C.c_void_p]),
    'dmh_photo_guide_dev': (c_int, [C.c_void_p, c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p, c_float, C.c_void_p, c_f32p,
                                    c_int, c_int, c_int, C.c_void_p]),
    'dmh_photo_energy': (c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p, c_int, c_int, c_int, C.c_void_p]),
    'dmh_flow_guidance_shift': (c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, c_float, c_int, c_i64, C.c_void_p]),
    'dmh_affine_rows_keep': (c_int, [c_f32p, c_f32p, c_float, c_float, C.c_void_p, c_int, c_i64, C.c_void_p]),
    'dmh_attention_pag': (c_int, [c_f32p, c_f32p, c_int, c_int, c_float, C.c_void_p, c_int, C.c_void_p]),
    'dmh_pag_shift': (c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, c_float, c_int, c_i64, C.c_void_p]),
    'dmh_rng_indexed': (c_int, [c_f32p, c_int, c_i64, C.c_void_p, C.c_void_p, c_int, C.c_void_p]),
    'dmh_rng_keep_mask': (c_int, [C.c_void_p, c_int, C.c_void_p, C.c_void_p, c_float, C.c_void_p]),
    'dmh_rows_lincomb': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_i64, c_int, C.c_void_p]),
    'dmh_pixel_grid': (c_int, [c_f32p, c_int, c_int, c_int, c_float, C.c_void_p]),
    'dmh_norm_grid': (c_int, [c_f32p, c_f32p, c_int, c_int, c_int, C.c_void_p]),
    'dmh_homography_flow_points': (c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_int, c_int, c_int, c_int, c_int, C.c_void_p]),
    'dmh_dlt_points': (c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_int, c_int, C.c_void_p]),
    'dmh_affine': (c_int, [c_f32p, c_f32p, c_float, c_float, c_i64, C.c_void_p]),
    'dmh_affine_tail': (c_int, [c_f32p, c_int, c_int, c_int, c_int, c_float, c_float, C.c_void_p]),
    'dmh_q_sample': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_i64, C.c_void_p]),
    'dmh_diff_mean': (c_int, [c_f32p, c_f32p, c_f32p, c_int, C.c_void_p, c_f32p, c_int, c_int, c_int, C.c_void_p]),
    'dmh_loss_combine': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_int, C.c_void_p]),
    'dmh_to_uint8': (c_int, [c_f32p, C.c_void_p, c_i64, C.c_void_p]),
    'dmh_homography_flow': (c_int, [C.c_void_p, c_f32p, c_f32p, c_int, c_int, c_int, c_float, C.c_void_p]),
    'dmh_flow_to_image': (c_int, [c_f32p, c_f32p, c_int, c_int, c_float, C.c_void_p]),
    'dmh_flow_warp': (c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                              C.c_void_p]),
    'dmh_dlt_homography': (c_int, [c_f32p, C.c_void_p, C.c_void_p, c_int, c_int, c_int, C.c_void_p]),
    'dmh_post_process': (c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_int, c_int, c_int, C.c_void_p]),
    'dmh_preview_sheet': (c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                  C.c_void_p]),
    'dmh_homography_warp': (c_int, [c_f32p, C.c_void_p, c_f32p, c_int, c_int, c_int, c_int, c_int, C.c_void_p]),
    'dmh_hem_batch': (c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_int, c_int, c_int, c_int,
                              c_int, c_int, c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p]),
    'dmh_hem_flow': (c_int, [C.c_void_p, c_int, c_int, c_int, c_f32p, C.c_void_p]),
}

# name -> (restype, argtypes); the entries include/dmhomo_hip_known.h declares: the same library and error channel, a table of
# their own (SIGNATURES is the table of dmhomo_hip.h, whose version stays what it is)
EXTENSIONS = {
    'dmh_known_blend': (c_int, [c_f32p, c_f32p, C.c_void_p, c_float, c_f32p, C.c_void_p, c_f32p, c_int, c_i64, C.c_void_p]),
    'dmh_known_error_splits': (c_int, [c_int, c_i64]),
    'dmh_known_error': (c_int, [c_f32p, c_f32p, C.c_void_p, c_float, c_f32p, C.c_void_p, C.c_void_p, C.c_void_p, c_int, c_i64,
                                C.c_void_p]),
}

# name -> (restype, argtypes); the entry include/dmhomo_hip_start.h declares (sample_from's start image), in a table of its
# own for the same reason
START_EXTENSIONS = {
    'dmh_start_mix': (c_int, [c_f32p, c_f32p, C.c_void_p, C.c_void_p, c_float, c_float, c_f32p, c_int, c_i64, C.c_void_p]),
}

# name -> (restype, argtypes); the entry include/dmhomo_hip_relabel.h declares (ddpm.relabel_batch: a new homography label per
# sample, drawn on the device), in a table of its own for the same reason
RELABEL_EXTENSIONS = {
    'dmh_relabel_batch': (c_int, [c_f32p, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_double, c_float, C.c_void_p, c_int,
                                  c_f32p, C.c_void_p, C.c_void_p, c_int, c_int, c_int, C.c_void_p]),
}

DLT_BLOCKS = 64

_lib = None


class DmhError(RuntimeError):
    pass


def lib():
    """the loaded shared library; raises if it was not built (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DmhError(f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                           f'or `make -C dmhomo_amd/csrc` — dmhomo_amd has no CPU / eager fallback')
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(EXTENSIONS.items()) + list(START_EXTENSIONS.items()) + \
                list(RELABEL_EXTENSIONS.items()):
            fn = getattr(h, name)          # AttributeError if the symbol is missing (a stale library fails here, loudly)
            fn.restype = res
            fn.argtypes = args
        got = int(h.dmh_version())
        if got != ABI_VERSION:
            raise DmhError(f'{LIB_PATH} reports ABI version {got}, this binding was written against {ABI_VERSION} '
                           f'(include/dmhomo_hip.h): rebuild the library with `make -C dmhomo_amd/csrc`')
        _lib = h
    return _lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def graph_capture(graph, pool=None):
    """``torch.cuda.graph(graph, pool=pool, capture_error_mode='thread_local')`` with Python's cyclic collector kept out of
    the capture.  A dropped diffusion object or evicted capture is a reference cycle (entry -> step body -> entry) that
    holds HIP graphs and their memory pool; only the collector frees it, and where it happened to run inside a capture the
    graph and pool destructors called into HIP from the capturing thread, which a thread-local capture forbids: the process
    aborted.  (torch.cuda.graph collected on entry until torch 2.9; it no longer does.)  So: collect first, then hold the
    collector off until the capture has ended."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, pool=pool, capture_error_mode='thread_local'):
            yield
    finally:
        if was_enabled:
            gc.enable()


def call(name, *args):
    """invoke an int-returning entry point on torch's current stream; raise on a DMH_E* code."""
    h = lib()
    rc = getattr(h, name)(*args, stream())
    if rc != 0:
        raise DmhError(f'{name} failed ({rc}): {h.dmh_last_error().decode()}')


def ptr(t, dtype=torch.float32):
    """device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise DmhError('dmhomo_amd kernels need tensors on the GPU (got a CPU tensor); there is no CPU path')
    if dtype is not None and t.dtype != dtype:
        raise DmhError(f'expected dtype {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise DmhError('expected a contiguous tensor')
    return C.c_void_p(t.data_ptr())
