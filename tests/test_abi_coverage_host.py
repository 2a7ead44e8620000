"""Every entry of the C ABI (dmhomo_amd/_lib.py: SIGNATURES) names the test file that launches it ALONE — through
``ops.call`` / the ctypes handle by its own name, or through the thin ``ops`` wrapper the row gives — so that a new entry
cannot be added without a test of its own being pointed at.  Size queries, dmh_version and dmh_last_error may point at
tests/test_cabi.py or at the host file that holds them against a restated plan.  A row marked COMPOSITE has no alone-test:
it names the composite that reaches the entry; those rows are printed and their number is capped at what was found when
the table was filled."""
import os
import re

from dmhomo_amd import _lib

TESTS = os.path.dirname(os.path.abspath(__file__))
COMPOSITE = 'composite-only'

# entry -> (files, names looked for in each file: the entry itself if empty, note)
_T = {}


def _row(entries, files, names=(), note=''):
    for e in entries.split():
        assert e not in _T, e
        _T[e] = (tuple(files.split()), tuple(names), note)


_row('dmh_last_error dmh_version dmh_conv_pack_floats dmh_conv_tiles dmh_linattn_splits', 'test_cabi.py')
_row('dmh_conv_up2_pack_floats', 'test_gpu_weight_image.py', ('ops.PackedConv',))
_row('dmh_ws_standardize', 'test_gpu_kernels.py', ('ops.ws_standardize',))
_row('dmh_pack_conv_weight dmh_pack_conv_weight_up2', 'test_gpu_weight_image.py', ('ops.PackedConv',))
_row('dmh_pack_conv_weights_multi', 'test_gpu_weight_image.py', ('ops.PackBatch',))
_row('dmh_conv2d', 'test_gpu_conv_fwd.py')
_row('dmh_rows_from_keep', 'test_gpu_interval.py test_gpu_dedup.py')
_row('dmh_gn_finalize dmh_gn_finalize_bound dmh_gn_silu_residual dmh_gn_silu_residual_stats dmh_chan_layernorm '
     'dmh_pixel_stats dmh_sinusoidal_embed dmh_fourier_embed dmh_assemble_input dmh_final_conv_nchw dmh_sampler_seek '
     'dmh_rows_lincomb dmh_affine dmh_affine_tail dmh_q_sample dmh_diff_mean dmh_loss_combine dmh_to_uint8',
     'test_gpu_fwd_glue.py')
_row('dmh_class_embed', 'test_gpu_fwd_glue.py', ('ops.class_embed',))
_row('dmh_ss_gather', 'test_gpu_fwd_glue.py', ('ops.ss_gather',))
_row('dmh_linattn_partial_floats dmh_linattn_context dmh_linattn_merge dmh_linattn_apply dmh_linattn_merge_ms '
     'dmh_linattn_bwd_workspace_floats dmh_linattn_backward dmh_attention', 'test_gpu_attn_core.py')
_row('dmh_conv_wgrad_workspace_floats', 'test_wgrad_splits_host.py test_grad_conv_host.py')
_row('dmh_conv_wgrad', 'test_gpu_grad_conv.py test_gpu_wgrad_splits.py test_gpu_backward.py')
_row('dmh_conv_unshuffle_wgrad_workspace_floats', 'test_ddp_train_host.py test_grad_conv_host.py')
_row('dmh_conv_unshuffle_wgrad', 'test_gpu_grad_conv.py test_gpu_ddp_train.py')
_row('dmh_s2d_shift dmh_d2s dmh_sumpool2 dmh_loss_backward dmh_loss_backward_ddp dmh_sumsq dmh_gradnorm_finalize dmh_adam '
     'dmh_adam_multi dmh_sumsq_multi dmh_ema dmh_resize_bilinear_u8 dmh_mask_open_nearest dmh_pixel_grid dmh_norm_grid '
     'dmh_homography_flow_points dmh_homography_flow dmh_flow_to_image', 'test_gpu_aux.py')
_row('dmh_sumsq_blocks', 'test_gpu_aux.py', ('ops.sumsq_blocks',))
_row('dmh_gn_finalize_train dmh_gn_silu_backward dmh_sum_over_batch dmh_bgemm dmh_softmax_rows dmh_softmax_rows_backward',
     'test_gpu_norm_backward.py')
_row('dmh_gn_bwd_chunks dmh_lnb_blocks', 'test_norm_backward_host.py')
_row('dmh_ws_backward', 'test_gpu_norm_backward.py', ('ops.ws_backward',))
_row('dmh_chan_layernorm_backward', 'test_gpu_norm_backward.py', ('ops.chan_layernorm_backward',))
_row('dmh_act', 'test_gpu_wgrad_splits.py', ('ops.act',))
_row('dmh_class_embed_backward', 'test_gpu_wgrad_splits.py')
_row('dmh_multi_blocks', 'test_asan_host.py')
_row('dmh_linattn_fused_pack_floats dmh_linattn_fused_pack', 'test_gpu_linattn_fused.py', ('ops.PackedLinAttn',))
_row('dmh_linattn_out_pack_floats dmh_linattn_out_pack', 'test_gpu_linattn_fused.py', ('ops.PackedLinAttnOut',))
_row('dmh_linattn_fused_splits dmh_linattn_fused_context dmh_linattn_fused_apply_out dmh_linattn_merge_n '
     'dmh_linattn_fused_apply', 'test_gpu_linattn_fused.py')
_row('dmh_linear', 'test_gpu_kernels.py')
_row('dmh_sampler_step dmh_sampler_step_dev dmh_sampler_step_ddp_dev', 'test_gpu_kernels.py')
_row('dmh_sampler_step_ms dmh_sampler_step_ddp_ms_dev', 'test_gpu_solver.py')
_row('dmh_sampler_step_ms_dev', 'test_gpu_solver.py', ('ops.sampler_step_ms_dev',))
_row('dmh_row_quantile_abs dmh_sampler_threshold dmh_sampler_step_thr dmh_sampler_step_thr_dev', 'test_gpu_threshold.py')
_row('dmh_sampler_threshold_dev', 'test_gpu_threshold.py', ('ops.sampler_threshold_dev',))
_row('dmh_guidance_splits', 'test_guidance_host.py')
_row('dmh_guidance_factor dmh_sampler_threshold_gr dmh_sampler_step_gr', 'test_gpu_guidance.py')
_row('dmh_guidance_factor_dev', 'test_gpu_guidance.py', ('ops.guidance_factor_dev',))
_row('dmh_sampler_threshold_gr_dev', 'test_gpu_guidance.py', ('ops.sampler_threshold_gr_dev',))
_row('dmh_sampler_step_gr_dev', 'test_gpu_guidance.py', ('ops.sampler_step_gr_dev',))
_row('dmh_rows_gated dmh_guidance_gate', 'test_gpu_interval.py')
_row('dmh_apg_splits', 'test_apg_host.py')
_row('dmh_apg_coef dmh_apg_apply', 'test_gpu_apg.py')
_row('dmh_apg_coef_dev', 'test_gpu_apg.py', ('ops.apg_coef_dev',))
_row('dmh_photo_acc_words dmh_photo_energy_splits', 'test_photo_host.py')
_row('dmh_photo_weights dmh_photo_guide dmh_photo_energy', 'test_gpu_photo.py')
_row('dmh_photo_guide_dev', 'test_gpu_photo.py', ('ops.photo_guide_dev',))
_row('dmh_flow_guidance_shift', 'test_gpu_flowg.py', ('ops.flow_guidance_shift',))
_row('dmh_affine_rows_keep', 'test_gpu_flowg.py', ('ops.affine_rows_keep',))
_row('dmh_attention_pag dmh_pag_shift', 'test_gpu_pag.py')
_row('dmh_rng_indexed dmh_rng_keep_mask', 'test_gpu_rng.py')
_row('dmh_dlt_points', 'test_gpu_surface.py', ('ddp.DLT_solve',),
     'ddpm.DLT_solve is the thin wrapper of ops.dlt_points; held to 1e-10 of the reference\'s pinv on explicit point sets')
_row('dmh_flow_warp', 'test_gpu_geometry.py test_gpu_aux.py', ('ops.flow_warp', 'dmh_flow_warp'))
_row('dmh_dlt_homography', 'test_gpu_geometry.py')
_row('dmh_post_process dmh_preview_sheet dmh_homography_warp', 'test_gpu_preview.py')
_row('dmh_hem_batch dmh_hem_flow', 'test_gpu_hem_data.py')

COMPOSITE_ONLY_FOUND = 0        # rows marked COMPOSITE when the table was filled: the cap


def test_table_has_one_row_per_entry():
    missing = sorted(set(_lib.SIGNATURES) - set(_T))
    extra = sorted(set(_T) - set(_lib.SIGNATURES))
    assert not missing, f'C-ABI entries without a row (name the test that launches each alone): {missing}'
    assert not extra, f'rows for entries that SIGNATURES no longer has: {extra}'


def test_named_files_exist_and_name_the_entry():
    for entry, (files, names, _) in _T.items():
        assert files, entry
        want = names or (entry,)
        for f in files:
            path = os.path.join(TESTS, f)
            assert os.path.isfile(path), f'{entry}: tests/{f} does not exist'
            text = open(path).read()
            assert any(re.search(r'(?<!\w)' + re.escape(n) + r'\b', text) for n in want), \
                f'{entry}: tests/{f} names none of {want}'


def test_composite_only_rows_are_capped():
    rows = {e: note for e, (_, _, note) in _T.items() if note.startswith(COMPOSITE)}
    for e, note in rows.items():
        print(f'[coverage] {e}: {note}')
    print(f'[coverage] {len(rows)} of {len(_T)} entries are composite-only, cap {COMPOSITE_ONLY_FOUND}')
    assert len(rows) <= COMPOSITE_ONLY_FOUND, sorted(rows)
