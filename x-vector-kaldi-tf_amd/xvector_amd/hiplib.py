"""ctypes binding of ``libxvector_hip.so`` (the C ABI declared in ``include/xvector_hip.h``).

There is NO fallback: if the shared library is missing, or no MI355X is visible, every entry point
raises.  torch is imported first so that the library's ``libamdhip64.so.7`` dependency resolves to the
HIP runtime torch already loaded (same SONAME) -- device pointers of torch tensors are then valid in
the kernels, and torch's current stream can be passed straight through.
"""
import ctypes
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("XVECTOR_HIP_LIB") or os.path.join(_HERE, "libxvector_hip.so")     # override: kernel experiments
ABI_VERSION = 44

# every entry point include/xvector_hip.h declares, in its order: name -> (restype, argtypes)
_vp, _ci, _cf, _i64, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64, ctypes.c_size_t
_SIGNATURES = {
    "xv_version": (_ci, []),
    "xv_last_error": (ctypes.c_char_p, []),
    "xv_set_tuning": (_ci, [_ci, _ci]),
    "xv_pack_weights_f32": (_ci, [_vp, _ci, _ci, _vp, _vp]),
    "xv_fold_bn_f32": (_ci, [_vp, _vp, _vp, _vp, _cf, _ci, _vp, _vp, _vp]),
    "xv_fold_shift_taps_f32": (_ci, [_vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp]),
    "xv_tdnn_layer_f32": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _vp]),
    "xv_packed_weights_rows_f32_floats": (_sz, [_ci, _ci, _ci, _ci]),
    "xv_pack_weights_rows_f32": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _vp]),
    "xv_tdnn_layer_rows_f32": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _vp, _vp, _ci, _vp]),
    # "fp32tc": the wide-context layers with fewer multiplications (Toom-Cook F(2, K) over time)
    "xv_toom_supported": (_ci, [_ci, _ci, _ci, _ci]),
    "xv_packed_weights_toom_f32_floats": (_sz, [_ci, _ci, _ci]),
    "xv_pack_weights_toom_f32": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp]),
    "xv_tdnn_layer_toom_f32": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _vp, _vp, _ci, _vp]),
    "xv_tdnn_layer_toom_dilated_f32": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _ci, _vp]),
    # bf16x3 split-precision twins
    "xv_packed_weights_bf16x3_bytes": (_sz, [_ci, _ci, _ci]),
    "xv_pack_weights_bf16x3": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp]),
    "xv_pack_weights_bf16x3_many": (_ci, [_ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xv_split_row_bytes": (_sz, [_ci]),
    "xv_split_encode_f32": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp]),
    "xv_split_decode_f32": (_ci, [_vp, _i64, _ci, _vp, _ci, _vp]),
    "xv_tdnn_layer_bf16x3": (_ci, [_vp, _ci, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _ci, _ci, _vp, _ci, _vp]),
    "xv_tdnn_layer_bf16x3_sums": (_ci, [_vp, _ci, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _ci, _vp, _vp]),
    "xv_tdnn_layer_bf16x3_moments": (_ci, [_vp, _ci, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _ci, _vp, _vp]),
    "xv_block_stats_bytes": (_sz, [_i64, _ci]),
    "xv_tdnn_layer_pool_bf16x3": (_ci, [_vp, _ci, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp]),
    "xv_stats_pool_blocks_f32": (_ci, [_vp, _ci, _vp, _vp, _ci, _cf, _vp, _vp]),
    "xv_tdnn_layer_pool_f32": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp]),
    "xv_packed_first_bf16x3_bytes": (_sz, [_ci, _ci, _ci]),
    "xv_pack_first_bf16x3": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp]),
    "xv_tdnn_first_bf16x3": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp]),
    "xv_packed_pair_bf16x3_bytes": (_sz, [_ci, _ci, _ci]),
    "xv_pack_pair_bf16x3": (_ci, [_vp, _vp, _ci, _ci, _ci, _vp, _vp]),
    "xv_tdnn_pair_pool_bf16x3": (_ci, [_vp, _i64, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp]),
    # f16bf8 split-precision twins of the hidden frame-level layers
    "xv_packed_weights_f16bf8_bytes": (_sz, [_ci, _ci, _ci]),
    "xv_pack_weights_f16bf8": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp]),
    "xv_split8_encode_f32": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp, _vp]),
    "xv_split8_decode_f32": (_ci, [_vp, _i64, _ci, _vp, _ci, _vp]),
    "xv_tdnn_layer_f16bf8": (_ci, [_vp, _i64, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _ci, _vp, _vp]),
    "xv_tdnn_layer_pool_f16bf8": (_ci, [_vp, _i64, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp]),
    "xv_tdnn_first_f16bf8": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp]),
    "xv_tdnn_first_f16mx6": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp]),
    "xv_packed_pair_f16bf8_bytes": (_sz, [_ci, _ci, _ci]),
    "xv_pack_pair_f16bf8": (_ci, [_vp, _vp, _ci, _ci, _ci, _vp, _vp]),
    "xv_tdnn_pair_pool_f16bf8": (_ci, [_vp, _i64, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp]),
    "xv_packed_pair_f16mx6_bytes": (_sz, [_ci, _ci, _ci]),
    "xv_pack_pair_f16mx6": (_ci, [_vp, _vp, _ci, _ci, _ci, _vp, _vp]),
    "xv_tdnn_pair_pool_f16mx6": (_ci, [_vp, _i64, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp]),
    # a hidden layer's cross terms on e2m3 MFMAs: the XV_FMT_SPLIT6 activation format, its weights and its layer
    "xv_packed_weights_f16mx6_bytes": (_sz, [_ci, _ci, _ci]),
    "xv_pack_weights_f16mx6": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp]),
    "xv_split6_encode_f32": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp, _vp]),
    "xv_split6_decode_f32": (_ci, [_vp, _i64, _ci, _vp, _vp, _ci, _vp]),
    "xv_tdnn_layer_f16mx6": (_ci, [_vp, _i64, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _ci, _vp, _vp]),
    "xv_fc_bf16x3": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp]),
    "xv_stats_pool_workspace_bytes": (_sz, [_ci, _ci, _ci, _ci]),
    "xv_stats_pool_f32": (_ci, [_vp, _i64, _ci, _vp, _vp, _ci, _ci, _ci, _cf, _vp, _vp, _vp]),
    "xv_fc_f32": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp]),
    "xv_fc_splitk_workspace_bytes": (_sz, [_ci, _ci, _ci]),
    "xv_fc_splitk_f32": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp]),
    "xv_chunk_average_f32": (_ci, [_vp, _vp, _vp, _ci, _ci, _vp, _vp]),
    # training step
    "xv_chunk_moments_f32": (_ci, [_vp, _i64, _ci, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp]),
    "xv_merge_moments_f32": (_ci, [_vp, _vp, _ci, _ci, _vp, _vp, _vp]),
    "xv_rows_affine_f32": (_ci, [_vp, _ci, _i64, _ci, _vp, _vp, _vp, _vp, _ci, _vp]),
    "xv_rows_affine_split_f32": (_ci, [_vp, _ci, _i64, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _vp]),
    "xv_wgrad_workspace_bytes": (_sz, [_i64, _ci, _ci, _ci]),
    "xv_wgrad_f32": (_ci, [_vp, _ci, _vp, _ci, _i64, _ci, _ci, _ci, _ci, _vp, _vp, _vp]),
    "xv_wgrad_bf16x3": (_ci, [_vp, _ci, _vp, _ci, _i64, _ci, _ci, _ci, _ci, _vp, _vp, _vp]),
    "xv_wgrad_bias_workspace_bytes": (_sz, [_i64, _ci, _ci, _ci]),
    "xv_wgrad_bias_bf16x3": (_ci, [_vp, _ci, _vp, _ci, _i64, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp]),
    "xv_col_sums_workspace_bytes": (_sz, [_i64, _ci]),
    "xv_col_sums_f32": (_ci, [_vp, _ci, _vp, _ci, _i64, _ci, _vp, _vp, _vp, _vp]),
    "xv_bn_act_backward_f32": (_ci, [_vp, _vp, _ci, _i64, _ci, _vp, _vp, _vp, _vp, _vp, _cf, _cf, _ci, _cf, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xv_bn_act_backward_split_f32": (_ci, [_vp, _vp, _ci, _i64, _ci, _vp, _vp, _vp, _vp, _vp, _cf, _cf, _ci, _cf, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xv_bn_act_backward_parts_f32": (_ci, [_vp, _vp, _ci, _i64, _ci, _vp, _vp, _vp, _vp, _cf, _cf, _ci, _cf, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xv_bn_moments_fold_f32": (_ci, [_vp, _i64, _ci, _cf, _vp, _vp, _cf, _vp, _vp, _vp, _vp, _vp]),
    "xv_col_sums_merge_f32": (_ci, [_vp, _i64, _ci, _vp, _vp, _vp]),
    "xv_pool_bn_act_backward_f32": (_ci, [_vp, _vp, _ci, _ci, _vp, _vp, _ci, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _cf, _cf, _ci, _cf, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xv_bn_small_forward_f32": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp, _cf, _vp, _vp, _vp, _ci, _vp]),
    "xv_bn_small_backward_f32": (_ci, [_vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _cf, _ci, _cf, _vp, _vp, _vp, _vp]),
    "xv_pool_backward_f32": (_ci, [_vp, _ci, _ci, _vp, _vp, _ci, _i64, _vp, _vp, _vp, _vp]),
    "xv_softmax_ce_f32": (_ci, [_vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp]),
    "xv_adam_f32": (_ci, [_vp, _vp, _vp, _vp, _i64, _cf, _cf, _cf, _cf, _vp]),
    "xv_axpy_f32": (_ci, [_vp, _vp, _cf, _i64, _vp]),
    "xv_sumsq_workspace_bytes": (_sz, [_i64]),
    "xv_sumsq_f32": (_ci, [_vp, _i64, _vp, _vp, _vp]),
    "xv_dropout_f32": (_ci, [_vp, _ci, _i64, _ci, ctypes.c_uint64, _cf, _vp]),
    "xv_minibatch_layout": (_ci, [_ci, _ci, _ci, _i64, _vp, _vp, _vp, _vp]),
    "xv_pack_minibatch_f32": (_ci, [_vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _i64, _vp]),
    "xv_prelu_backward_f32": (_ci, [_vp, _vp, _ci, _i64, _ci, _vp, _vp]),
    "xv_ema_f32": (_ci, [_vp, _vp, _ci, _cf, _vp]),
    # additive-margin softmax head
    "xv_l2_normalize_rows_f32": (_ci, [_vp, _ci, _ci, _ci, _vp, _ci, _vp, _vp]),
    "xv_l2_normalize_backward_f32": (_ci, [_vp, _vp, _vp, _ci, _ci, _vp, _vp]),
    "xv_am_margin_f32": (_ci, [_vp, _vp, _ci, _ci, _cf, _cf, _vp]),
    # self-attentive statistics pooling
    "xv_attention_scores_f32": (_ci, [_vp, _i64, _i64, _ci, _vp, _vp, _vp, _i64, _vp]),
    "xv_attention_softmax_f32": (_ci, [_vp, _vp, _vp, _ci, _vp, _vp]),
    "xv_attention_pool_workspace_bytes": (_sz, [_ci, _ci, _ci, _ci]),
    "xv_attention_pool_f32": (_ci, [_vp, _i64, _ci, _vp, _vp, _vp, _ci, _ci, _ci, _cf, _vp, _vp, _vp]),
    "xv_attention_pool_backward_f32": (_ci, [_vp, _i64, _ci, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _i64, _vp, _vp]),
    "xv_attention_softmax_backward_f32": (_ci, [_vp, _vp, _vp, _vp, _ci, _vp, _vp]),
    "xv_attention_scores_backward_f32": (_ci, [_vp, _i64, _vp, _vp, _i64, _ci, _vp, _i64, _vp]),
    # feature front-end
    "xv_cmn_sliding_scatter_f32": (_ci, [_vp, _ci, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _ci, _vp]),
    # PLDA / cosine scoring back-end
    "xv_backend_prepare_f32": (_ci, [_vp, _i64, _ci, _ci, _vp, _vp, _vp, _i64, _vp, _ci, _ci, _vp, _vp, _vp, _ci, _vp, _i64, _vp, _vp]),
    "xv_score_matrix_f32": (_ci, [_vp, _vp, _i64, _ci, _ci, _ci, _vp, _vp, _i64, _vp]),
    "xv_score_blocks_f32": (_ci, [_vp, _vp, _i64, _ci, _ci, _vp, _vp, _vp, _ci, _ci, _vp, _i64, _vp, _vp]),
    "xv_score_pairs_f32": (_ci, [_vp, _vp, _i64, _ci, _vp, _vp, _i64, _vp, _vp, _vp]),
    "xv_topk_row_stats_f32": (_ci, [_vp, _i64, _ci, _ci, _ci, _vp, _vp, _vp]),
    # moments for PLDA adaptation
    "xv_moment_stats_f64": (_ci, [_vp, _i64, _i64, _ci, _vp, _vp, _i64, _vp, _sz, _vp]),
    "xv_moment_stats_workspace_bytes": (_sz, [_i64, _ci]),
    # clustering for PLDA adaptation
    "xv_ahc_average_f64": (_ci, [_vp, _i64, _ci, ctypes.c_double, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "xv_ahc_average_workspace_bytes": (_sz, [_ci]),
    # diarization: one clustering problem per recording
    "xv_ahc_average_batch_f64": (_ci, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "xv_ahc_average_batch_workspace_bytes": (_sz, [_ci]),
    # diarization: per-recording PCA and the PLDA projected into it
    "xv_pca_plda_groups_f64": (_ci, [_vp, _i64, _ci, _vp, _ci, _ci, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _sz, _vp]),
    "xv_pca_plda_groups_workspace_bytes": (_sz, [_ci, _ci]),
    "xv_backend_prepare_groups_f32": (_ci, [_vp, _i64, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _i64, _vp, _vp, _vp]),
    # diarization: VBx resegmentation of every recording's vectors
    "xv_vbx_groups_f64": (_ci, [_vp, _i64, _ci, _vp, _ci, _ci, _vp, _vp, _vp, _ci, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double,
                                ctypes.c_double, ctypes.c_double, _ci, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "xv_vbx_groups_workspace_bytes": (_sz, [_ci, _ci, _ci, _ci]),
    "xv_mfcc_f32": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp, _ci, _i64, _vp, _vp, _vp, _vp, _ci, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _ci,
                          _cf, _cf, _ci, _ci, _ci, _cf, _vp, _i64, _vp, _i64, _vp]),
    "xv_vad_energy_f32": (_ci, [_vp, _i64, _vp, _vp, _ci, _cf, _cf, _ci, _cf, _vp, _vp]),
    # stage 2: wav-reverberate
    "xv_augment_power_f64": (_ci, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "xv_augment_conv_f64": (_ci, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "xv_augment_gains_f32": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xv_augment_mix_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "xv_augment_level_f32": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp]),
    "xv_augment_write": (_ci, [_vp, _vp, _vp, _vp, _i64, _vp, _ci, _vp, _vp]),
    # stages 3-5: training examples
    "xv_vad_compact_i32": (_ci, [_vp, _vp, _vp, _ci, _i64, _vp, _vp, _vp]),
    "xv_egs_chunks_f16": (_ci, [_vp, _ci, _ci, _i64, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _i64, _vp]),
    # the extractor's destination-row plan from device-resident VAD decisions
    "xv_voiced_rank_i32": (_ci, [_vp, _vp, _vp, _ci, _i64, _vp, _vp, _vp]),
    "xv_chunk_row_plan_i32": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp]),
    # compressed feature output
    "xv_cm_payload_bytes": (_i64, [_ci, _ci]),
    "xv_cm_encode_f32": (_ci, [_vp, _i64, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp]),
    # sample-rate conversion in front of the MFCC kernel
    "xv_resample_num_output": (_i64, [_i64, _ci, _ci]),
    "xv_resample_f32": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    # SPHERE audio (G.711, big-endian PCM) decoded in front of the MFCC kernel
    "xv_wave_decode": (_ci, [_vp, _i64, _vp, _ci, _vp, _i64, _vp, _ci, _vp]),
    # sliding-window extraction: the packed rows of overlapping sub-segments
    "xv_cmn_sliding_gather_f32": (_ci, [_vp, _ci, _ci, _i64, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp,
                                        _ci, _i64, _vp]),
    # speech segments from device-resident VAD decisions
    "xv_vad_segments_i32": (_ci, [_vp, _vp, _vp, _ci, _i64, _ci, _ci, _ci, _ci, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "xv_vad_segments_workspace_bytes": (_sz, [_i64]),
    "xv_vad_segments_capacity": (_i64, [_i64, _ci, _ci, _ci]),
}
SYMBOLS = tuple(_SIGNATURES)      # tests check the header declares exactly these and the .so exports all of them

FMT_F32, FMT_SPLIT, FMT_SPLIT8, FMT_SPLIT6 = 0, 1, 2, 3
SPLIT_PAD_BEFORE, SPLIT_PAD_AFTER = 8, 264
TUNE_TILE_ROWS = 1
TUNE_FIRST_TILES = 2
TUNE_FP32_GEMM = 3

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_PRELU = 0, 1, 2, 3

BACKEND_KSTEP = 8
SIDE_PLAIN, SIDE_ENROL, SIDE_TEST, SIDE_COSINE = 0, 1, 2, 3
MOMENT_SLAB = 2048                # XV_MOMENT_SLAB: rows per partial of xv_moment_stats_f64
MOMENT_DIM_MAX = 256
AHC_MAX_N = 32768                  # XV_AHC_MAX_N: items of one xv_ahc_average_f64 call
AHC_BATCH_MAX_N = 4096             # XV_AHC_BATCH_MAX_N: items of one group of xv_ahc_average_batch_f64
PCA_MAX_DIM = 128                  # XV_PCA_MAX_DIM: the vector dimension of xv_pca_plda_groups_f64
PCA_MAX_SWEEPS = 30                # XV_PCA_MAX_SWEEPS: the sweep cap of its Jacobi iteration
VBX_MAX_SPK = 64                   # XV_VBX_MAX_SPK: speakers of one group of xv_vbx_groups_f64
VBX_MAX_ITERS = 100                # XV_VBX_MAX_ITERS: its iteration cap
SEG_TILE = 256                     # XV_SEG_TILE: frames per step of xv_vad_segments_i32

_lib = None


class XvectorHipError(RuntimeError):
    pass


def load():
    """Load the shared library (no GPU needed for loading / symbol checks)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise XvectorHipError("HIP extension not built: %s is missing (run `python -c 'import __graft_entry__ as g; "
                              "g.build()'` or `make -C x-vector-kaldi-tf_amd/csrc`)" % SO_PATH)
    import torch  # noqa: F401  (loads torch's libamdhip64 first; see module docstring)
    lib = ctypes.CDLL(SO_PATH)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.xv_version() != ABI_VERSION:
        raise XvectorHipError("libxvector_hip.so ABI version %d != expected %d" % (lib.xv_version(), ABI_VERSION))
    _lib = lib
    return lib


_GPU_SEEN = []


def require_gpu():
    """Load the library and insist on a visible GPU.  Called by every compute entry point.  (Only the POSITIVE answer is
    remembered: a training step makes ~150 calls, and torch.cuda.is_available() behind each of them was a tenth of the host
    time of a step; without a GPU every call still raises.)"""
    if _GPU_SEEN:
        return _GPU_SEEN[0]
    lib = load()
    import torch
    if not torch.cuda.is_available():
        raise XvectorHipError("no MI355X visible (torch.cuda.is_available() is False): the x-vector hot path "
                              "has no CPU fallback")
    _GPU_SEEN.append(lib)
    return lib


def set_tuning(key, value):
    """Process-wide launch tuning (``TUNE_*`` keys of the header); never changes results."""
    lib = load()
    _check(lib.xv_set_tuning(int(key), int(value)), "xv_set_tuning")


def _check(rc, what):
    if rc != 0:
        raise XvectorHipError("%s failed (%d): %s" % (what, rc, load().xv_last_error().decode()))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_RAW_STREAM = []


def _stream():
    """The HIP stream torch considers current on the current device (the launches of this package go where torch's own work
    goes).  Through torch's raw-stream accessor when it has one: building a torch.cuda.Stream object per launch was a fifth of
    the host time of a training step."""
    import torch
    if not _RAW_STREAM:
        _RAW_STREAM.append(getattr(torch._C, "_cuda_getCurrentRawStream", None))
    raw = _RAW_STREAM[0]
    if raw is not None:
        return ctypes.c_void_p(raw(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------
# argument checks: what keeps a wrong shape or a host tensor from a kernel that trusts its arguments
# ------------------------------------------------------------------------------------------------
# strictness of _f32: contiguous (any rank); 2-D with dense rows (a column slice of a wider buffer passes, its stride(0) goes to
# the kernel as the leading dimension); the same with stride(0) >= shape[1] (no overlapping rows)
_DENSE, _ROWS, _ROWS_LD = 0, 1, 2
_F32_WHAT = ("%s must be a contiguous cuda float32 tensor", "%s must be cuda float32 rows",
             "%s must be a 2-D cuda float32 tensor with dense rows")


def _f32(t, name, level=_DENSE):
    import torch
    assert t.is_cuda and t.dtype == torch.float32 and (
        t.is_contiguous() if level == _DENSE else
        t.dim() == 2 and t.stride(1) == 1 and (level == _ROWS or t.stride(0) >= t.shape[1])), _F32_WHAT[level] % name
    return t


_rows2d = functools.partial(_f32, level=_ROWS)          # _rows2d(t, name) / _f32_rows(t, name): the two stricter levels by name
_f32_rows = functools.partial(_f32, level=_ROWS_LD)


def _dev(t, dtype, name, n=None):
    """Pointer of a contiguous cuda tensor of ``dtype`` (index tables, fp64 accumulators, ...) of at least ``n`` elements."""
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), "%s must be a contiguous cuda %s tensor" % (name, dtype)
    assert n is None or t.numel() >= n, "%s must hold at least %d elements" % (name, n)
    return _ptr(t)


def _chunk_tables(row_start, row_len):
    """The per-chunk tables of the pooling kernels.  (Dtype and device only, as every copy of this check had it: not _dev's
    contiguity test.)"""
    import torch
    assert row_start.dtype == torch.int32 and row_len.dtype == torch.int32 and row_start.is_cuda and row_len.is_cuda


def _valid(row_valid, R):
    """Pointer of the optional row mask of ``R`` rows: one byte per row, on the device."""
    assert row_valid is None or (row_valid.is_cuda and row_valid.numel() >= R and row_valid.element_size() == 1), \
        "row_valid must be a cuda tensor of at least %d one-byte elements" % R
    return _ptr(row_valid)


def _operand(t, channels, R, name, fmts, level=_ROWS):
    """(pointer, leading dimension, format) of an activation operand of ``channels`` channels and at least ``R`` rows.  ``fmts``
    lists what the kernel takes: FMT_SPLIT / FMT_SPLIT8 for a SplitBuf in that format (leading dimension 0), FMT_F32 for fp32
    rows (checked by _f32 at ``level``), None where the operand may be left out."""
    if t is None:
        assert None in fmts, "%s is required" % name
        return None, 0, FMT_F32
    if isinstance(t, SplitBuf):
        assert t.fmt in fmts and t.channels == channels and t.rows >= R, \
            "%s: a split buffer in one of the formats %s with %d channels and at least %d rows is expected" % (name, fmts, channels, R)
        return ctypes.c_void_p(t.ptr), 0, t.fmt
    assert FMT_F32 in fmts, "%s must be a SplitBuf" % name
    _f32(t, name, level)
    assert t.shape[1] == channels and t.shape[0] >= R, "%s must be [>= %d, %d]" % (name, R, channels)
    return _ptr(t), t.stride(0), FMT_F32


def _split_out(buf, c, R):
    """Pointer of the optional bf16-split second output (``c`` channels, at least ``R`` rows) of an element-wise kernel."""
    return _operand(buf, c, R, "split output", (FMT_SPLIT, None))[0]


def _nbytes(t):
    return t.numel() * t.element_size()


def _ws(nbytes, device):
    import torch
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)


def _scale_shift(like):
    """Uninitialised (scale, shift) of a BN fold, one float per element of ``like`` (gamma)."""
    import torch
    c = like.numel()
    return torch.empty(c, dtype=torch.float32, device=like.device), torch.empty(c, dtype=torch.float32, device=like.device)


def _bn_coef(c, device):
    """The [3, c] coefficient scratch the BN-backward kernels fill and read back in one launch."""
    import torch
    return torch.empty(3 * c, dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------------------
# thin wrappers over the ABI, operating on torch-ROCm tensors (device memory + stream plumbing only)
# ------------------------------------------------------------------------------------------------
def pack_weights(w2d):
    """w2d: [Kred, Cout] -> packed [Cout, Kred]."""
    import torch
    lib = require_gpu()
    _f32(w2d, "w")
    kred, cout = w2d.shape
    wp = torch.empty((cout, kred), dtype=torch.float32, device=w2d.device)
    _check(lib.xv_pack_weights_f32(_ptr(w2d), kred, cout, _ptr(wp), _stream()), "xv_pack_weights_f32")
    return wp


class _Packed(object):
    """Packed weights of one kernel form + the shape they were packed for: the constructor takes the attributes a subclass
    names in ``__slots__``, in that order."""
    __slots__ = ()

    def __init__(self, *values):
        assert len(values) == len(self.__slots__)
        for k, v in zip(self.__slots__, values):
            setattr(self, k, v)


def _pack_bytes(size_fn, pack_fn, name, cls, tensors, dims, unsupported=None):
    """A packing that lives in a byte buffer: ``size_fn(*dims)`` bytes are allocated, ``pack_fn`` (the entry point ``name``) fills
    them from ``tensors``, and ``cls(buffer, *dims)`` comes back.  ``unsupported``: format of ``dims`` for the error raised when
    the library reports 0 bytes (None: left to the entry point, which names what it does not take)."""
    import torch
    dims = tuple(int(v) for v in dims)
    nbytes = int(size_fn(*dims))
    if unsupported is not None and nbytes == 0:
        raise XvectorHipError("%s: unsupported shape %s" % (name, unsupported % dims))
    wt = torch.empty(nbytes, dtype=torch.uint8, device=tensors[0].device)
    _check(pack_fn(*[_ptr(t) for t in tensors], *dims, _ptr(wt), _stream()), name)
    return cls(wt, *dims)


class PackedRows(_Packed):
    """Weights of a first layer for the "rows" form (xv_pack_weights_rows_f32): wp[Cout, roundup32(K ldx)] for feature rows of ldx floats."""
    __slots__ = ("wp", "K", "cin", "ldx", "cout")


def pack_weights_rows(w3d, ldx):
    """w3d: TF layout [K, Cin, Cout] (cuda float32), ldx: floats per packed feature row (>= Cin, a multiple of 4) -> PackedRows."""
    import torch
    lib = require_gpu()
    _f32(w3d, "w")
    K, cin, cout = w3d.shape
    n = int(lib.xv_packed_weights_rows_f32_floats(K, cin, int(ldx), cout))
    assert n > 0, "rows form unsupported for K=%d Cin=%d ldx=%d" % (K, cin, ldx)
    wp = torch.empty((cout, n // cout), dtype=torch.float32, device=w3d.device)
    _check(lib.xv_pack_weights_rows_f32(_ptr(w3d), K, cin, int(ldx), cout, _ptr(wp), _stream()), "xv_pack_weights_rows_f32")
    return PackedRows(wp, K, cin, int(ldx), cout)


def tdnn_layer_rows(x, w, bias, scale, shift, act, alpha, row_valid, y, rows=None):
    """xv_tdnn_layer_rows_f32: x[R, ldx] contiguous feature rows -> y[R, Cout] fp32 rows, w a PackedRows."""
    lib = require_gpu()
    _rows2d(x, "x")
    R = x.shape[0] if rows is None else int(rows)
    assert x.shape[1] == w.ldx and x.stride(0) == w.ldx and y.shape[1] == w.cout and y.shape[0] >= R
    _check(lib.xv_tdnn_layer_rows_f32(_ptr(x), R, w.cin, w.ldx, _ptr(w.wp), _ptr(bias), _ptr(scale), _ptr(shift), int(act), _ptr(alpha),
                                      w.K, w.cout, _valid(row_valid, R), _ptr(y), y.stride(0), _stream()), "xv_tdnn_layer_rows_f32")


class PackedToom(_Packed):
    """Transformed taps of one K in {3, 5, 7} layer for the Toom-Cook F(2, K) kernel (xv_pack_weights_toom_f32): wp[Cout, (K+1) Cin]."""
    __slots__ = ("wp", "K", "cin", "cout")


def toom_supported(K, dilation, cin, cout):
    return bool(load().xv_toom_supported(int(K), int(dilation), int(cin), int(cout)))


def pack_weights_toom(w3d):
    """w3d: TF layout [K, Cin, Cout] (cuda float32) -> PackedToom."""
    import torch
    lib = require_gpu()
    _f32(w3d, "w")
    K, cin, cout = w3d.shape
    n = int(lib.xv_packed_weights_toom_f32_floats(K, cin, cout))
    assert n > 0, "Toom-Cook form unsupported for K=%d Cin=%d Cout=%d" % (K, cin, cout)
    wp = torch.empty((cout, (K + 1) * cin), dtype=torch.float32, device=w3d.device)
    _check(lib.xv_pack_weights_toom_f32(_ptr(w3d), K, cin, cout, _ptr(wp), _stream()), "xv_pack_weights_toom_f32")
    return PackedToom(wp, K, cin, cout)


def tdnn_layer_toom(x, w, bias, scale, shift, act, alpha, row_valid, y, rows=None, dilation=1):
    """xv_tdnn_layer_toom_dilated_f32: x[R, Cin] -> y[R, Cout] fp32 rows, w a PackedToom (chunks on multiples of 2 * dilation rows)."""
    lib = require_gpu()
    _rows2d(x, "x")
    R = x.shape[0] if rows is None else int(rows)
    assert x.shape[1] == w.cin and y.shape[1] == w.cout and y.shape[0] >= R
    if int(dilation) == 1:
        _check(lib.xv_tdnn_layer_toom_f32(_ptr(x), R, w.cin, x.stride(0), _ptr(w.wp), _ptr(bias), _ptr(scale), _ptr(shift), int(act),
                                          _ptr(alpha), w.K, w.cout, _valid(row_valid, R), _ptr(y), y.stride(0), _stream()),
               "xv_tdnn_layer_toom_f32")
        return
    _check(lib.xv_tdnn_layer_toom_dilated_f32(_ptr(x), R, w.cin, x.stride(0), _ptr(w.wp), _ptr(bias), _ptr(scale), _ptr(shift), int(act),
                                              _ptr(alpha), w.K, int(dilation), w.cout, _valid(row_valid, R), _ptr(y), y.stride(0),
                                              _stream()), "xv_tdnn_layer_toom_dilated_f32")


class Packed3(_Packed):
    """Tiled bf16x3 weights of one layer (xv_pack_weights_bf16x3) + the shape they were packed for."""
    __slots__ = ("wt", "K", "cin", "cout")


def pack_weights_bf16x3(w3d):
    """w3d: [K, Cin, Cout] fp32 (TF layout; FC: [1, In, Out]) -> Packed3."""
    lib = require_gpu()
    return _pack_bytes(lib.xv_packed_weights_bf16x3_bytes, lib.xv_pack_weights_bf16x3, "xv_pack_weights_bf16x3", Packed3,
                       (_f32(w3d, "w"),), w3d.shape)


class PackPlan(object):
    """The bf16x3 tiles of several layers, forward and (optionally) input-gradient orientation, re-packed by ONE launch
    (xv_pack_weights_bf16x3_many) into one persistent device buffer: what a training step does after every optimizer update.
    ``layers``: [(w3d [K, Cin, Cout] fp32 device tensor -- a VIEW whose storage the optimizer updates in place --, cin_pad, want_bwd)]."""

    def __init__(self, layers):
        import torch
        lib = require_gpu()
        n = len(layers)
        self.n = n
        dev = layers[0][0].device
        sizes, offs, total = [], [], 0
        for w, cin_pad, want_bwd in layers:
            _f32(w, "w")
            K, cin, cout = w.shape
            assert cin_pad >= cin
            f = int(lib.xv_packed_weights_bf16x3_bytes(K, cin_pad, cout))
            b = int(lib.xv_packed_weights_bf16x3_bytes(K, cout, cin_pad)) if want_bwd else 0
            offs.append((total, total + f))
            total += f + b
            sizes.append((f, b))
        self.buf = torch.empty(total, dtype=torch.uint8, device=dev)
        base = self.buf.data_ptr()
        assert base % 16 == 0
        arr_p, arr_i = ctypes.c_void_p * n, ctypes.c_int32 * n
        self._w = arr_p(*[w.data_ptr() for w, _, _ in layers])
        self._K = arr_i(*[int(w.shape[0]) for w, _, _ in layers])
        self._cin = arr_i(*[int(w.shape[1]) for w, _, _ in layers])
        self._pad = arr_i(*[int(c) for _, c, _ in layers])
        self._cout = arr_i(*[int(w.shape[2]) for w, _, _ in layers])
        self._fwd = arr_p(*[base + o[0] for o in offs])
        self._bwd = arr_p(*[(base + o[1]) if sz[1] else None for o, sz in zip(offs, sizes)])
        self._keep = [w for w, _, _ in layers]
        self.fwd, self.bwd = [], []
        for (w, cin_pad, want_bwd), o, sz in zip(layers, offs, sizes):
            K, cin, cout = w.shape
            self.fwd.append(Packed3(self.buf[o[0]:o[0] + sz[0]], K, cin_pad, cout))
            self.bwd.append(Packed3(self.buf[o[1]:o[1] + sz[1]], K, cout, cin_pad) if want_bwd else None)

    def repack(self):
        lib = require_gpu()
        _check(lib.xv_pack_weights_bf16x3_many(self.n, self._w, self._K, self._cin, self._pad, self._cout, self._fwd, self._bwd,
                                               _stream()), "xv_pack_weights_bf16x3_many")


class SplitBuf(object):
    """Device buffer in a split activation format (``fmt``: FMT_SPLIT = bf16 hi/lo planes, FMT_SPLIT8 = fp16 hi + bf8
    cross bytes, FMT_SPLIT6 = fp16 hi + e2m3 cross blocks; same geometry) with the zero padding rows the layer kernels may read
    (rows [-SPLIT_PAD_BEFORE, rows + SPLIT_PAD_AFTER))."""

    def __init__(self, rows, channels, device, fmt=FMT_SPLIT):
        import torch
        self.rows, self.channels, self.fmt = int(rows), int(channels), int(fmt)
        self.row_bytes = int(load().xv_split_row_bytes(self.channels))
        self.base = torch.zeros((SPLIT_PAD_BEFORE + self.rows + SPLIT_PAD_AFTER) * self.row_bytes, dtype=torch.uint8, device=device)
        self.ptr = self.base.data_ptr() + SPLIT_PAD_BEFORE * self.row_bytes      # row 0

    def view(self, channels, fmt=None):
        """Same storage seen as a buffer of ``channels`` channels per row (<= allocated width), optionally in another
        split format (all-zero bytes are zeros in all of them)."""
        v = object.__new__(SplitBuf)
        v.rows, v.channels, v.base = self.rows, int(channels), self.base
        v.fmt = self.fmt if fmt is None else int(fmt)
        v.row_bytes = int(load().xv_split_row_bytes(v.channels))
        assert v.row_bytes <= self.row_bytes
        v.ptr = self.base.data_ptr() + SPLIT_PAD_BEFORE * v.row_bytes
        return v


def split_encode(x, buf, rows=None, status=None):
    """fp32 rows x[R, C] -> buf (SplitBuf, any format; ``status``: int32 device tensor, FMT_SPLIT8 / FMT_SPLIT6 only)."""
    lib = require_gpu()
    _f32(x, "x")
    R = x.shape[0] if rows is None else int(rows)
    assert R <= buf.rows and x.shape[1] == buf.channels
    if buf.fmt in (FMT_SPLIT8, FMT_SPLIT6):
        name = "xv_split8_encode_f32" if buf.fmt == FMT_SPLIT8 else "xv_split6_encode_f32"
        _check(getattr(lib, name)(_ptr(x), R, x.shape[1], x.stride(0), ctypes.c_void_p(buf.ptr), _ptr(status), _stream()), name)
        return
    _check(lib.xv_split_encode_f32(_ptr(x), R, x.shape[1], x.stride(0), ctypes.c_void_p(buf.ptr), _stream()), "xv_split_encode_f32")


def split_decode(buf, rows, out=None, cq=None):
    """SplitBuf -> fp32 tensor [rows, C].  ``cq`` (FMT_SPLIT6 only): a tensor like ``out`` (same row stride) that receives the
    dequantised second cross-term operand."""
    import torch
    lib = require_gpu()
    if out is None:
        out = torch.empty((rows, buf.channels), dtype=torch.float32, device=buf.base.device)
    if buf.fmt == FMT_SPLIT6:
        assert cq is None or (cq.shape == out.shape and cq.stride(0) == out.stride(0))
        _check(lib.xv_split6_decode_f32(ctypes.c_void_p(buf.ptr), int(rows), buf.channels, _ptr(out), _ptr(cq), out.stride(0), _stream()),
               "xv_split6_decode_f32")
        return out
    assert cq is None
    name = "xv_split8_decode_f32" if buf.fmt == FMT_SPLIT8 else "xv_split_decode_f32"
    _check(getattr(lib, name)(ctypes.c_void_p(buf.ptr), int(rows), buf.channels, _ptr(out), out.stride(0), _stream()), name)
    return out


def tdnn_layer3(x, R, w, bias, scale, shift, act, alpha, dilation, row_valid, y, y_preact=None):
    """bf16x3 layer.  x / y: contiguous fp32 tensors [>=R, C] (XV_FMT_F32) or SplitBuf (XV_FMT_SPLIT); w: Packed3."""
    lib = require_gpu()
    assert isinstance(w, Packed3)
    xp, ldx, xfmt = _operand(x, w.cin, R, "x", (FMT_F32, FMT_SPLIT))
    yp, ldy, yfmt = _operand(y, w.cout, R, "y", (FMT_F32, FMT_SPLIT, None))
    prep, ldpre, _ = _operand(y_preact, w.cout, R, "y_preact", (FMT_F32, None), _DENSE)      # contiguous: stricter than y, as before
    _check(lib.xv_tdnn_layer_bf16x3(xp, xfmt, int(R), w.cin, ldx, _ptr(w.wt), _ptr(bias), _ptr(scale), _ptr(shift), int(act),
                                    _ptr(alpha), w.K, int(dilation), w.cout, _valid(row_valid, R), yp, yfmt, ldy, prep, ldpre,
                                    _stream()), "xv_tdnn_layer_bf16x3")


def col_sums_workspace(rows, c, device):
    """Partial-sum workspace of xv_col_sums_f32 / xv_tdnn_layer_bf16x3_sums: [ceil(rows / 128)][2][c] doubles."""
    return _ws(load().xv_col_sums_workspace_bytes(int(rows), int(c)), device)


def tdnn_layer3_sums(x, R, w, dilation, row_valid, y, sum_r, workspace):
    """xv_tdnn_layer_bf16x3_sums: the plain GEMM y = x * w (no bias / activation: the input-gradient GEMM of the training step),
    fp32 rows out, and per 128-row tile the partial column sums [sum y | sum y * sum_r] in ``workspace`` (col_sums_workspace)."""
    lib = require_gpu()
    assert isinstance(w, Packed3) and supports_sums(w.cout)
    xp, ldx, xfmt = _operand(x, w.cin, R, "x", (FMT_F32, FMT_SPLIT))
    yp, ldy, _ = _operand(y, w.cout, R, "y", (FMT_F32,))
    sp, lds, _ = _operand(sum_r, w.cout, R, "sum_r", (FMT_F32,))
    _check(lib.xv_tdnn_layer_bf16x3_sums(xp, xfmt, int(R), w.cin, ldx, _ptr(w.wt), None, None, None, ACT_NONE, None, w.K, int(dilation),
                                         w.cout, _valid(row_valid, R), yp, ldy, sp, lds, _ptr(workspace), _stream()),
           "xv_tdnn_layer_bf16x3_sums")


def supports_sums(cout):
    return cout % 8 == 0


def tdnn_layer3_moments(x, R, w, bias, act, alpha, dilation, row_valid, y, y_preact, workspace):
    """xv_tdnn_layer_bf16x3_moments: the forward layer r = act(conv(x, w) + b) with fp32 rows out (+ the pre-activation), and per
    128-row tile the partial sums [sum r | sum r^2] in ``workspace`` (col_sums_workspace) -- BN's batch moments (bn_moments_fold)."""
    lib = require_gpu()
    assert isinstance(w, Packed3) and supports_sums(w.cout)
    xp, ldx, xfmt = _operand(x, w.cin, R, "x", (FMT_F32, FMT_SPLIT))
    yp, ldy, _ = _operand(y, w.cout, R, "y", (FMT_F32,))
    prep, ldpre, _ = _operand(y_preact, w.cout, R, "y_preact", (FMT_F32, None), _DENSE)      # contiguous: stricter than y, as before
    _check(lib.xv_tdnn_layer_bf16x3_moments(xp, xfmt, int(R), w.cin, ldx, _ptr(w.wt), _ptr(bias), None, None, int(act), _ptr(alpha), w.K,
                                            int(dilation), w.cout, _valid(row_valid, R), yp, ldy, prep, ldpre, _ptr(workspace),
                                            _stream()), "xv_tdnn_layer_bf16x3_moments")


def bn_moments_fold(workspace, rows, n_frames, gamma, beta, eps, mean, var):
    """(scale, shift) of the BN fold and the batch moments (into mean, var) from the partial sums of tdnn_layer3_moments."""
    lib = require_gpu()
    c = gamma.numel()
    scale, shift = _scale_shift(gamma)
    _check(lib.xv_bn_moments_fold_f32(_ptr(workspace), int(rows), c, float(n_frames), _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")),
                                      float(eps), _ptr(_f32(mean, "mean")), _ptr(_f32(var, "var")), _ptr(scale), _ptr(shift), _stream()),
           "xv_bn_moments_fold_f32")
    return scale, shift


POOL_BLOCK_ROWS = 8      # chunks fed to tdnn_layer_pool must start on a multiple of this many rows


def block_stats_floats(rows, cout):
    return int(load().xv_block_stats_bytes(int(rows), int(cout))) // 4


def _block_stats(block_stats, R, cout):
    """Pointer of the block-statistics output of ``R`` rows of ``cout`` channels."""
    assert _f32(block_stats, "block_stats").numel() >= block_stats_floats(R, cout), "block_stats too small"
    return _ptr(block_stats)


def tdnn_layer_pool(x, R, w, bias, scale, shift, act, alpha, dilation, row_valid, block_stats, K=None):
    """Last frame-level layer with the block-statistics epilogue: block_stats = flat fp32 tensor of
    >= block_stats_floats(R, cout) elements, laid out [ceil(R/8)][2][Cout].  w: Packed3 (bf16x3) or the packed fp32 weights
    of pack_weights() together with ``K`` (exact fp32, x: fp32 rows)."""
    lib = require_gpu()
    if not isinstance(w, Packed3):
        _rows2d(x, "x"); _f32(w, "wp")
        cin, cout = x.shape[1], w.shape[0]
        assert K is not None and w.shape[1] == int(K) * cin and x.shape[0] >= R
        _check(lib.xv_tdnn_layer_pool_f32(_ptr(x), int(R), cin, x.stride(0), _ptr(w), _ptr(bias), _ptr(scale), _ptr(shift), int(act),
                                          _ptr(alpha), int(K), int(dilation), cout, _valid(row_valid, R),
                                          _block_stats(block_stats, R, cout), _stream()), "xv_tdnn_layer_pool_f32")
        return
    xp, ldx, fmt = _operand(x, w.cin, R, "x", (FMT_F32, FMT_SPLIT), _DENSE)      # contiguous x: stricter than tdnn_layer3, as before
    _check(lib.xv_tdnn_layer_pool_bf16x3(xp, fmt, int(R), w.cin, ldx, _ptr(w.wt), _ptr(bias), _ptr(scale), _ptr(shift), int(act),
                                         _ptr(alpha), w.K, int(dilation), w.cout, _valid(row_valid, R),
                                         _block_stats(block_stats, R, w.cout), _stream()), "xv_tdnn_layer_pool_bf16x3")


class PackedFirst(_Packed):
    """Weights of the first frame-level layer in the fragment order of xv_tdnn_first_bf16x3."""
    __slots__ = ("wt", "K", "cin", "cout")


def first_supported(K, cin, cout):
    return int(load().xv_packed_first_bf16x3_bytes(int(K), int(cin), int(cout))) > 0


def pack_first_bf16x3(w3d):
    """w[K, Cin, Cout] (device fp32, TF order) -> PackedFirst."""
    lib = require_gpu()
    _f32(w3d, "w"); assert w3d.dim() == 3
    return _pack_bytes(lib.xv_packed_first_bf16x3_bytes, lib.xv_pack_first_bf16x3, "xv_pack_first_bf16x3", PackedFirst, (w3d,), w3d.shape,
                       unsupported="K=%d, %d -> %d")


def tdnn_first(x, R, w, bias, scale, shift, act, alpha, dilation, row_valid, y, status=None):
    """First frame-level layer: x fp32 rows [>=R, ld] (ld % 8 == 0, columns >= Cin zero) -> y (SplitBuf; its format selects
    the entry point, ``status`` as for tdnn_layer8).  w: PackedFirst."""
    lib = require_gpu()
    assert isinstance(w, PackedFirst) and isinstance(y, SplitBuf)
    _rows2d(x, "x"); assert x.shape[0] >= R and x.shape[1] >= w.cin
    assert y.channels == w.cout and y.rows >= R
    if y.fmt in (FMT_SPLIT8, FMT_SPLIT6):
        name = "xv_tdnn_first_f16bf8" if y.fmt == FMT_SPLIT8 else "xv_tdnn_first_f16mx6"
        _check(getattr(lib, name)(_ptr(x), int(R), w.cin, x.stride(0), _ptr(w.wt), _ptr(bias), _ptr(scale), _ptr(shift), int(act),
                                  _ptr(alpha), w.K, int(dilation), w.cout, _valid(row_valid, R), ctypes.c_void_p(y.ptr),
                                  _ptr(status), _stream()), name)
        return
    _check(lib.xv_tdnn_first_bf16x3(_ptr(x), int(R), w.cin, x.stride(0), _ptr(w.wt), _ptr(bias), _ptr(scale), _ptr(shift), int(act),
                                    _ptr(alpha), w.K, int(dilation), w.cout, _valid(row_valid, R), ctypes.c_void_p(y.ptr), _stream()),
           "xv_tdnn_first_bf16x3")


class Packed8(_Packed):
    """Tiled f16bf8 weights of one layer (xv_pack_weights_f16bf8) + the shape they were packed for."""
    __slots__ = ("wt", "K", "cin", "cout")


def f16bf8_supported(K, dilation):
    """Shapes xv_tdnn_layer_f16bf8 takes (the split-input shapes of the bf16x3 kernel)."""
    span = (int(K) - 1) * int(dilation)
    return int(K) in (1, 3, 5, 7) and (int(K) == 1 or 2 <= span <= 8)


def pack_weights_f16bf8(w3d):
    """w3d: [K, Cin, Cout] fp32 (TF layout) -> Packed8."""
    lib = require_gpu()
    return _pack_bytes(lib.xv_packed_weights_f16bf8_bytes, lib.xv_pack_weights_f16bf8, "xv_pack_weights_f16bf8", Packed8,
                       (_f32(w3d, "w"),), w3d.shape)


def _tap_bias(tapbias, w):
    """The [K, Cout] table of fold_shift_taps for the layer packed as ``w`` (None: none)."""
    if tapbias is not None:
        _f32(tapbias, "tapbias")
        assert tuple(tapbias.shape) == (w.K, w.cout), "tapbias must be [K, Cout] = [%d, %d]" % (w.K, w.cout)
    return _ptr(tapbias)


def tdnn_layer8(x, R, w, bias, scale, shift, act, alpha, dilation, row_valid, y, status=None, tapbias=None):
    """f16bf8 layer.  x: SplitBuf in FMT_SPLIT8; y: contiguous fp32 tensor [>=R, C] or SplitBuf of any format (FMT_SPLIT6: the
    16 x 16 MFMA form of the 256 x 256 tile only -- layer_mx6_supported); w: Packed8 -- or PackedMx6 with x in FMT_SPLIT6: the
    same layer with its cross terms on e2m3 MFMAs (tdnn_layer_mx6);
    status: int32 device tensor whose bit 0 is set when a FMT_SPLIT8 output had to be clamped (None: not reported);
    tapbias: the per-tap constants of fold_shift_taps when x was stored without its BN shift (``bias`` is then bias_full)."""
    lib = require_gpu()
    assert isinstance(w, (Packed8, PackedMx6))
    if isinstance(w, PackedMx6):
        return _layer8("xv_tdnn_layer_f16mx6", FMT_SPLIT6, lib, x, R, w, bias, scale, shift, act, alpha, dilation, row_valid, y, status, tapbias)
    _layer8("xv_tdnn_layer_f16bf8", FMT_SPLIT8, lib, x, R, w, bias, scale, shift, act, alpha, dilation, row_valid, y, status, tapbias)


def _layer8(name, xfmt, lib, x, R, w, bias, scale, shift, act, alpha, dilation, row_valid, y, status, tapbias):
    """The launch tdnn_layer8 and tdnn_layer_mx6 share: entry point ``name`` with x in ``xfmt``."""
    xp = _operand(x, w.cin, R, "x", (xfmt,))[0]
    yp, ldy, yfmt = _operand(y, w.cout, R, "y", (FMT_F32, FMT_SPLIT, FMT_SPLIT8, FMT_SPLIT6))
    _check(getattr(lib, name)(xp, int(R), w.cin, _ptr(w.wt), _ptr(bias), _ptr(scale), _ptr(shift), int(act), _ptr(alpha), w.K,
                              int(dilation), w.cout, _valid(row_valid, R), _tap_bias(tapbias, w), yp, yfmt, ldy, _ptr(status),
                              _stream()), name)


class PackedMx6(_Packed):
    """Tiled f16mx6 weights of one layer (xv_pack_weights_f16mx6) + the shape they were packed for."""
    __slots__ = ("wt", "K", "cin", "cout")


def layer_mx6_supported(K, dilation, cin, cout):
    """Shapes xv_tdnn_layer_f16mx6 takes: those of the 16 x 16 MFMA form of the 256 x 256 tile."""
    return f16bf8_supported(K, dilation) and int(load().xv_packed_weights_f16mx6_bytes(int(K), int(cin), int(cout))) > 0


def pack_weights_f16mx6(w3d):
    """w3d: [K, Cin, Cout] fp32 (TF layout) -> PackedMx6."""
    lib = require_gpu()
    return _pack_bytes(lib.xv_packed_weights_f16mx6_bytes, lib.xv_pack_weights_f16mx6, "xv_pack_weights_f16mx6", PackedMx6,
                       (_f32(w3d, "w"),), w3d.shape, unsupported="K = %d, %d -> %d")


def tdnn_layer_mx6(x, R, w, bias, scale, shift, act, alpha, dilation, row_valid, y, status=None, tapbias=None):
    """tdnn_layer8 with the cross terms on block-scaled e2m3 MFMAs: x: SplitBuf in FMT_SPLIT6 (written by a layer's epilogue);
    w: PackedMx6; y: a SplitBuf of any format."""
    lib = require_gpu()
    assert isinstance(w, PackedMx6)
    _layer8("xv_tdnn_layer_f16mx6", FMT_SPLIT6, lib, x, R, w, bias, scale, shift, act, alpha, dilation, row_valid, y, status, tapbias)


def tdnn_layer_pool8(x, R, w, bias, scale, shift, act, alpha, dilation, row_valid, block_stats, tapbias=None):
    """tdnn_layer_pool in the f16bf8 arithmetic (x: SplitBuf in FMT_SPLIT8, w: Packed8; tapbias: as tdnn_layer8)."""
    lib = require_gpu()
    assert isinstance(w, Packed8)
    xp = _operand(x, w.cin, R, "x", (FMT_SPLIT8,))[0]
    _check(lib.xv_tdnn_layer_pool_f16bf8(xp, int(R), w.cin, _ptr(w.wt), _ptr(bias), _ptr(scale), _ptr(shift), int(act), _ptr(alpha), w.K,
                                         int(dilation), w.cout, _valid(row_valid, R), _tap_bias(tapbias, w),
                                         _block_stats(block_stats, R, w.cout), _stream()),
           "xv_tdnn_layer_pool_f16bf8")


class PackedPair(_Packed):
    """Weights of two consecutive K = 1 layers in the stage order of xv_tdnn_pair_pool_bf16x3."""
    __slots__ = ("wt", "cin", "cmid", "cout")


def pair_supported(cin, cmid, cout):
    return int(load().xv_packed_pair_bf16x3_bytes(int(cin), int(cmid), int(cout))) > 0


def _pack_pair(arith, cls, w1, w2):
    """The pair packing of an arithmetic ("bf16x3" / "f16bf8" / "f16mx6": the suffix of its entry points)."""
    lib = require_gpu()
    _f32(w1, "w1"); _f32(w2, "w2")
    assert w1.dim() == 2 and w2.dim() == 2 and w1.shape[1] == w2.shape[0]
    return _pack_bytes(getattr(lib, "xv_packed_pair_%s_bytes" % arith), getattr(lib, "xv_pack_pair_" + arith), "xv_pack_pair_" + arith,
                       cls, (w1, w2), (w1.shape[0], w1.shape[1], w2.shape[1]), unsupported="%d -> %d -> %d")


def _pair_pool(arith, cls, fmt, x, R, w, p1, p2, act, row_valid, block_stats, *status):
    """The pair launch of an arithmetic: ``w`` a ``cls``, ``x`` a SplitBuf in ``fmt``; ``status``: the extra pointer argument
    of the f16bf8 and f16mx6 entry points."""
    lib = require_gpu()
    assert isinstance(w, cls)
    xp = _operand(x, w.cin, R, "x", (fmt,))[0]
    name = "xv_tdnn_pair_pool_" + arith
    _check(getattr(lib, name)(xp, int(R), w.cin, w.cmid, w.cout, _ptr(w.wt), _ptr(p1[0]), _ptr(p1[1]), _ptr(p1[2]), _ptr(p1[3]),
                              _ptr(p2[0]), _ptr(p2[1]), _ptr(p2[2]), _ptr(p2[3]), int(act), _valid(row_valid, R),
                              _block_stats(block_stats, R, w.cout), *status, _stream()), name)


def pack_pair_bf16x3(w1, w2):
    """w1[Cin, Cmid], w2[Cmid, Cout] (device fp32, TF's [in, out] order) -> PackedPair."""
    return _pack_pair("bf16x3", PackedPair, w1, w2)


class PackedPair8(_Packed):
    """Weights of two consecutive K = 1 layers in the stage order of xv_tdnn_pair_pool_f16bf8."""
    __slots__ = ("wt", "cin", "cmid", "cout")


def pair8_supported(cin, cmid, cout):
    return int(load().xv_packed_pair_f16bf8_bytes(int(cin), int(cmid), int(cout))) > 0


def pack_pair_f16bf8(w1, w2):
    """w1[Cin, Cmid], w2[Cmid, Cout] (device fp32, TF's [in, out] order) -> PackedPair8."""
    return _pack_pair("f16bf8", PackedPair8, w1, w2)


def tdnn_pair_pool8(x, R, w, p1, p2, act, row_valid, block_stats, status=None):
    """tdnn_pair_pool in the f16bf8 arithmetic: x: SplitBuf in FMT_SPLIT8; w: PackedPair8; status: int32 device tensor (bit 0:
    the intermediate activation was clamped)."""
    _pair_pool("f16bf8", PackedPair8, FMT_SPLIT8, x, R, w, p1, p2, act, row_valid, block_stats, _ptr(status))


class PackedPairMx6(_Packed):
    """Weights of two consecutive K = 1 layers in the stage order of xv_tdnn_pair_pool_f16mx6 (the second layer's cross-term
    operands as e2m3 blocks)."""
    __slots__ = ("wt", "cin", "cmid", "cout")


def pair_mx6_supported(cin, cmid, cout):
    return int(load().xv_packed_pair_f16mx6_bytes(int(cin), int(cmid), int(cout))) > 0


def pack_pair_f16mx6(w1, w2):
    """w1[Cin, Cmid], w2[Cmid, Cout] (device fp32, TF's [in, out] order) -> PackedPairMx6."""
    return _pack_pair("f16mx6", PackedPairMx6, w1, w2)


def tdnn_pair_pool_mx6(x, R, w, p1, p2, act, row_valid, block_stats, status=None):
    """tdnn_pair_pool8 with the second layer's cross terms on block-scaled e2m3 MFMAs: x: SplitBuf in FMT_SPLIT8; w: PackedPairMx6."""
    _pair_pool("f16mx6", PackedPairMx6, FMT_SPLIT8, x, R, w, p1, p2, act, row_valid, block_stats, _ptr(status))


def tdnn_pair_pool(x, R, w, p1, p2, act, row_valid, block_stats):
    """Two K = 1 layers + pooling block statistics in one launch.  x: SplitBuf; w: PackedPair; p1 / p2: (bias, bn_scale,
    bn_shift, act_alpha) device tensors (None allowed) of the first / second layer."""
    _pair_pool("bf16x3", PackedPair, FMT_SPLIT, x, R, w, p1, p2, act, row_valid, block_stats)


def stats_pool_blocks(block_stats, c, row_start, row_len, nchunks, eps, out):
    lib = require_gpu()
    _f32(block_stats, "block_stats"); _f32(out, "out")
    _chunk_tables(row_start, row_len)
    assert out.shape[1] == 2 * c and out.shape[0] >= nchunks
    _check(lib.xv_stats_pool_blocks_f32(_ptr(block_stats), int(c), _ptr(row_start), _ptr(row_len), int(nchunks), float(eps),
                                        _ptr(out), _stream()), "xv_stats_pool_blocks_f32")


def fold_bn(gamma, beta, mean, var, eps):
    lib = require_gpu()
    c = gamma.numel()
    scale, shift = _scale_shift(gamma)
    _check(lib.xv_fold_bn_f32(_ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")), _ptr(_f32(mean, "mean")),
                              _ptr(_f32(var, "var")), float(eps), c, _ptr(scale), _ptr(shift), _stream()),
           "xv_fold_bn_f32")
    return scale, shift


def fold_shift_taps(w3d, shift, bias=None, table=True):
    """The share of a producer's BN ``shift[Cin]`` in the consumer with weights ``w3d[K, Cin, Cout]`` (device fp32):
    (tap[K, Cout] or None, bias_full[Cout]) with tap[t] = shift . w3d[t] and bias_full = bias + sum_t tap[t], in fp64."""
    lib = require_gpu()
    _f32(w3d, "w"); _f32(shift, "shift")
    K, cin, cout = (int(v) for v in w3d.shape)
    assert shift.numel() == cin and (bias is None or _f32(bias, "bias").numel() == cout)
    import torch
    tap = torch.empty((K, cout), dtype=torch.float32, device=w3d.device) if table else None
    full = torch.empty(cout, dtype=torch.float32, device=w3d.device)
    _check(lib.xv_fold_shift_taps_f32(_ptr(w3d), _ptr(shift), _ptr(bias), K, cin, cout, _ptr(tap), _ptr(full), _stream()),
           "xv_fold_shift_taps_f32")
    return tap, full


def tdnn_layer(x, wp, bias, scale, shift, act, alpha, K, dilation, row_valid, y, y_preact=None, rows=None):
    """x[R,Cin] -> y[R,Cout] (both contiguous 2-D cuda float32; only the first `rows` rows if given)."""
    lib = require_gpu()
    if isinstance(wp, Packed3):
        assert wp.K == K
        R = int(rows) if rows is not None else (x.rows if isinstance(x, SplitBuf) else x.shape[0])
        return tdnn_layer3(x, R, wp, bias, scale, shift, act, alpha, dilation, row_valid, y, y_preact)
    if isinstance(wp, PackedToom):
        assert wp.K == K and y_preact is None
        return tdnn_layer_toom(x, wp, bias, scale, shift, act, alpha, row_valid, y, rows, dilation)
    if isinstance(wp, PackedRows):
        assert wp.K == K and dilation == 1 and y_preact is None
        return tdnn_layer_rows(x, wp, bias, scale, shift, act, alpha, row_valid, y, rows)
    _rows2d(x, "x")
    _f32(wp, "wp")
    R = x.shape[0] if rows is None else int(rows)
    cin = x.shape[1]
    cout = wp.shape[0]
    assert wp.shape[1] == K * cin, "packed weight shape %s does not match K=%d Cin=%d" % (tuple(wp.shape), K, cin)
    out = y if y is not None else y_preact
    assert out.shape[1] == cout and out.shape[0] >= R
    if y is not None and y_preact is not None:
        assert y.shape[1] == y_preact.shape[1]
    _check(lib.xv_tdnn_layer_f32(_ptr(x), R, cin, x.stride(0), _ptr(wp), _ptr(bias), _ptr(scale), _ptr(shift), int(act),
                                 _ptr(alpha), int(K), int(dilation), cout, _valid(row_valid, R), _ptr(y), out.stride(0),
                                 _ptr(y_preact), _stream()), "xv_tdnn_layer_f32")


def stats_pool_workspace_bytes(c, nchunks, max_len, split_rows):
    return int(load().xv_stats_pool_workspace_bytes(int(c), int(nchunks), int(max_len), int(split_rows)))


def stats_pool(h, row_start, row_len, nchunks, max_len, split_rows, eps, out, workspace=None):
    lib = require_gpu()
    _f32(h, "h"); _f32(out, "out")
    _chunk_tables(row_start, row_len)
    c = h.shape[1]
    assert out.shape[1] == 2 * c and out.shape[0] >= nchunks
    need = stats_pool_workspace_bytes(c, nchunks, max_len, split_rows)
    if need:
        assert workspace is not None and _nbytes(workspace) >= need, "pool workspace too small"
    _check(lib.xv_stats_pool_f32(_ptr(h), h.stride(0), c, _ptr(row_start), _ptr(row_len), int(nchunks), int(max_len),
                                 int(split_rows), float(eps), _ptr(out), _ptr(workspace), _stream()), "xv_stats_pool_f32")


def fc(x, wp, bias, scale, shift, act, alpha, y, y_preact, rows=None):
    lib = require_gpu()
    _f32(x, "x")
    split = isinstance(wp, Packed3)
    if not split:
        _f32(wp, "wp")
    n = x.shape[0] if rows is None else int(rows)
    out_dim, in_dim = (wp.cout, wp.cin) if split else wp.shape
    assert x.shape[1] == in_dim
    for t in (y, y_preact):
        if t is not None:
            _f32(t, "y"); assert t.shape[1] == out_dim and t.shape[0] >= n
    if split:
        _check(lib.xv_fc_bf16x3(_ptr(x), n, in_dim, _ptr(wp.wt), _ptr(bias), _ptr(scale), _ptr(shift), int(act),
                                _ptr(alpha), out_dim, _ptr(y), _ptr(y_preact), _stream()), "xv_fc_bf16x3")
        return
    _check(lib.xv_fc_f32(_ptr(x), n, in_dim, _ptr(wp), _ptr(bias), _ptr(scale), _ptr(shift), int(act), _ptr(alpha),
                         out_dim, _ptr(y), _ptr(y_preact), _stream()), "xv_fc_f32")


def fc_splitk_supported(nrows, in_dim, out_dim):
    """Is ``[nrows, in_dim] -> out_dim`` skinny enough for the split-K form (xv_fc_splitk_f32)?"""
    return int(load().xv_fc_splitk_workspace_bytes(int(nrows), int(in_dim), int(out_dim))) > 0


def fc_splitk(x, wp, bias, scale, shift, act, alpha, y, y_preact):
    """xv_fc_splitk_f32: the exact-fp32 FC of a skinny problem with its reduction dealt to groups of workgroups (training
    minibatches' segment level).  wp: fp32 packed weights [Out, In] (pack_weights).  NOT used by extraction: the sum order
    differs from xv_fc_f32's, and an utterance's bits must not depend on the batch it is in."""
    lib = require_gpu()
    _f32(x, "x"); _f32(wp, "wp")
    n, in_dim = x.shape
    out_dim = wp.shape[0]
    assert wp.shape[1] == in_dim
    for t in (y, y_preact):
        if t is not None:
            _f32(t, "y"); assert t.shape[1] == out_dim and t.shape[0] >= n
    ws = _ws(lib.xv_fc_splitk_workspace_bytes(n, in_dim, out_dim), x.device)
    _check(lib.xv_fc_splitk_f32(_ptr(x), n, in_dim, _ptr(wp), _ptr(bias), _ptr(scale), _ptr(shift), int(act), _ptr(alpha), out_dim,
                                _ptr(y), _ptr(y_preact), _ptr(ws), _stream()), "xv_fc_splitk_f32")


def chunk_average(e, seg_start, chunk_len, nutts, out):
    import torch
    lib = require_gpu()
    _f32(e, "e"); _f32(out, "out")
    assert seg_start.dtype == torch.int32 and chunk_len.dtype == torch.int32
    dim = e.shape[1]
    assert out.shape[1] == dim and out.shape[0] >= nutts and seg_start.numel() >= nutts + 1
    _check(lib.xv_chunk_average_f32(_ptr(e), _ptr(seg_start), _ptr(chunk_len), int(nutts), dim, _ptr(out), _stream()),
           "xv_chunk_average_f32")


# ------------------------------------------------------------------------------------------------
# training-step wrappers
# ------------------------------------------------------------------------------------------------
def chunk_moments(h, row_start, row_len, nchunks, max_len, out, split_rows=512):
    """out[B, 2C] = per-chunk [mean || biased variance]."""
    lib = require_gpu()
    _f32(h, "h"); _f32(out, "out")
    c = h.shape[1]
    ws = _ws(stats_pool_workspace_bytes(c, nchunks, max_len, split_rows), h.device)
    _check(lib.xv_chunk_moments_f32(_ptr(h), h.stride(0), c, _ptr(row_start), _ptr(row_len), int(nchunks), int(max_len),
                                    int(split_rows), _ptr(out), _ptr(ws), _stream()), "xv_chunk_moments_f32")


def merge_moments(cm, row_len, nchunks, mean, var):
    lib = require_gpu()
    c = cm.shape[1] // 2
    _check(lib.xv_merge_moments_f32(_ptr(_f32(cm, "cm")), _ptr(row_len), int(nchunks), c, _ptr(mean), _ptr(var), _stream()),
           "xv_merge_moments_f32")


def rows_affine(x, scale, shift, row_valid, y, rows=None, y_split=None):
    """y_split: optional SplitBuf (bf16 split format) that receives a second copy of y."""
    lib = require_gpu()
    R = x.shape[0] if rows is None else int(rows)
    _check(lib.xv_rows_affine_split_f32(_ptr(_f32(x, "x")), x.stride(0), R, x.shape[1], _ptr(scale), _ptr(shift), _valid(row_valid, R),
                                        _ptr(_f32(y, "y")), y.stride(0), _split_out(y_split, x.shape[1], R), _stream()),
           "xv_rows_affine_split_f32")


def wgrad_takes_bias(precision, x, dz):
    """Whether ``wgrad(..., db=)`` can leave the bias gradient too (xv_wgrad_bias_bf16x3: bf16x3, 32-bit buffer offsets)."""
    return precision == "bf16x3" and x.shape[0] * x.stride(0) * 4 < 2 ** 31 and dz.shape[0] * dz.stride(0) * 4 < 2 ** 31


def wgrad(x, dz, K, dilation, dw, precision="fp32", db=None):
    """dw[K, Cin, Cout] (contiguous) = sum_r x[r + tap shift] (x) dz[r]; precision "fp32" (exact fp32 MFMA) or "bf16x3".
    ``db`` (bf16x3 only, see wgrad_takes_bias): also db[Cout] = sum_r dz[r], out of the rows the kernel streams anyway."""
    lib = require_gpu()
    fn, name = (lib.xv_wgrad_bf16x3, "xv_wgrad_bf16x3") if precision == "bf16x3" else (lib.xv_wgrad_f32, "xv_wgrad_f32")
    _rows2d(x, "x"); _rows2d(dz, "dz"); _f32(dw, "dw")
    R, cin = x.shape
    cout = dz.shape[1]
    assert dz.shape[0] == R and tuple(dw.shape) == (K, cin, cout)
    if db is not None:
        assert wgrad_takes_bias(precision, x, dz) and _f32(db, "db").numel() == cout
        ws = _ws(lib.xv_wgrad_bias_workspace_bytes(R, cin, cout, K), x.device)
        _check(lib.xv_wgrad_bias_bf16x3(_ptr(x), x.stride(0), _ptr(dz), dz.stride(0), R, cin, cout, int(K), int(dilation), _ptr(dw), _ptr(db),
                                        _ptr(ws), _stream()), "xv_wgrad_bias_bf16x3")
        return
    ws = _ws(lib.xv_wgrad_workspace_bytes(R, cin, cout, K), x.device)
    _check(fn(_ptr(x), x.stride(0), _ptr(dz), dz.stride(0), R, cin, cout, int(K), int(dilation), _ptr(dw), _ptr(ws), _stream()), name)


def col_sums(a, b, sum_a, sum_ab=None):
    lib = require_gpu()
    _f32(a, "a")
    R, c = a.shape
    ws = _ws(lib.xv_col_sums_workspace_bytes(R, c), a.device)
    _check(lib.xv_col_sums_f32(_ptr(a), a.stride(0), _ptr(b), b.stride(0) if b is not None else 0, R, c, _ptr(sum_a), _ptr(sum_ab),
                               _ptr(ws), _stream()), "xv_col_sums_f32")


def bn_act_backward(dh, r, sum_dh, sum_dh_r, mean, var, gamma, eps, n_frames, act, alpha, row_valid, dgamma, dbeta, dz, dz_split=None):
    """dz_split: optional SplitBuf (bf16 split format) that receives a second copy of dz."""
    lib = require_gpu()
    R, c = dh.shape
    coef = _bn_coef(c, dh.device)
    _check(lib.xv_bn_act_backward_split_f32(_ptr(_f32(dh, "dh")), _ptr(_f32(r, "r")), dh.stride(0), R, c, _ptr(sum_dh), _ptr(sum_dh_r),
                                            _ptr(mean), _ptr(var), _ptr(gamma), float(eps), float(n_frames), int(act), float(alpha),
                                            _valid(row_valid, R), _ptr(dgamma), _ptr(dbeta), _ptr(coef), _ptr(_f32(dz, "dz")),
                                            _split_out(dz_split, c, R), _stream()), "xv_bn_act_backward_split_f32")


def bn_act_backward_parts(dh, r, workspace, mean, var, gamma, eps, n_frames, act, alpha, row_valid, dgamma, dbeta, dz, dz_split=None):
    """bn_act_backward from the partial sums a producer left in ``workspace`` (tdnn_layer3_sums): no col_sums pass."""
    lib = require_gpu()
    R, c = dh.shape
    coef = _bn_coef(c, dh.device)
    _check(lib.xv_bn_act_backward_parts_f32(_ptr(_f32(dh, "dh")), _ptr(_f32(r, "r")), dh.stride(0), R, c, _ptr(workspace), _ptr(mean),
                                            _ptr(var), _ptr(gamma), float(eps), float(n_frames), int(act), float(alpha),
                                            _valid(row_valid, R), _ptr(dgamma), _ptr(dbeta), _ptr(coef), _ptr(_f32(dz, "dz")),
                                            _split_out(dz_split, c, R), _stream()), "xv_bn_act_backward_parts_f32")


BN_SMALL_MAX_ROWS = 1024


def bn_small_forward(x, gamma, beta, eps, mean, var, y):
    """xv_bn_small_forward_f32: training-mode BN of a matrix of <= 1024 rows in one launch (moments into mean / var, y = BN(x))."""
    lib = require_gpu()
    _rows2d(x, "x"); _rows2d(y, "y")
    n, c = x.shape
    assert n <= BN_SMALL_MAX_ROWS and y.shape == x.shape and gamma.numel() == c
    _check(lib.xv_bn_small_forward_f32(_ptr(x), x.stride(0), n, c, _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")), float(eps),
                                       _ptr(_f32(mean, "mean")), _ptr(_f32(var, "var")), _ptr(y), y.stride(0), _stream()),
           "xv_bn_small_forward_f32")


def bn_small_backward(dh, r, mean, var, gamma, eps, act, alpha, dgamma, dbeta, dz):
    """xv_bn_small_backward_f32: the BN + activation backward of a matrix of <= 1024 rows in one launch."""
    lib = require_gpu()
    _rows2d(dh, "dh"); _rows2d(r, "r"); _rows2d(dz, "dz")
    n, c = dh.shape
    assert n <= BN_SMALL_MAX_ROWS and r.shape == dh.shape == dz.shape and dh.stride(0) == r.stride(0) == dz.stride(0)
    _check(lib.xv_bn_small_backward_f32(_ptr(dh), _ptr(r), dh.stride(0), n, c, _ptr(mean), _ptr(var), _ptr(gamma), float(eps), int(act),
                                        float(alpha), _ptr(dgamma), _ptr(dbeta), _ptr(dz), _stream()), "xv_bn_small_backward_f32")


def col_sums_merge(workspace, rows, c, sum_a, sum_ab=None):
    _check(require_gpu().xv_col_sums_merge_f32(_ptr(workspace), int(rows), int(c), _ptr(sum_a), _ptr(sum_ab), _stream()),
           "xv_col_sums_merge_f32")


def pool_bn_act_backward(h, r, row_start, row_len, nchunks, pooled, dpooled, chunk_moments_r, mean, var, gamma, eps, n_frames, act, alpha,
                         dgamma, dbeta, dz, dz_split=None):
    """Backward of [statistics pooling -> BN -> activation] of the last frame-level layer (xv_pool_bn_act_backward_f32)."""
    lib = require_gpu()
    R, c = r.shape
    coef = _bn_coef(c, r.device)
    assert h.shape == r.shape and h.stride(0) == r.stride(0) == dz.stride(0)
    _check(lib.xv_pool_bn_act_backward_f32(_ptr(_f32(h, "h")), _ptr(_f32(r, "r")), r.stride(0), c, _ptr(row_start), _ptr(row_len),
                                           int(nchunks), R, _ptr(_f32(pooled, "pooled")), _ptr(_f32(dpooled, "dpooled")),
                                           _ptr(_f32(chunk_moments_r, "chunk_moments")), _ptr(mean), _ptr(var), _ptr(gamma), float(eps),
                                           float(n_frames), int(act), float(alpha), _ptr(dgamma), _ptr(dbeta), _ptr(coef),
                                           _ptr(_f32(dz, "dz")), _split_out(dz_split, c, R), _stream()), "xv_pool_bn_act_backward_f32")


def pool_backward(h, row_start, row_len, nchunks, pooled, dpooled, dh):
    lib = require_gpu()
    _check(lib.xv_pool_backward_f32(_ptr(_f32(h, "h")), h.stride(0), h.shape[1], _ptr(row_start), _ptr(row_len), int(nchunks),
                                    h.shape[0], _ptr(_f32(pooled, "pooled")), _ptr(_f32(dpooled, "dpooled")), _ptr(_f32(dh, "dh")),
                                    _stream()), "xv_pool_backward_f32")


def softmax_ce(logits, labels, loss_acc, dlogits=None):
    import torch
    lib = require_gpu()
    B, N = logits.shape
    assert labels.dtype == torch.int32
    ws = torch.empty(2 * B, dtype=torch.float32, device=logits.device)
    _check(lib.xv_softmax_ce_f32(_ptr(_f32(logits, "logits")), _ptr(labels), B, N, _ptr(loss_acc), _ptr(ws), _ptr(dlogits), _stream()),
           "xv_softmax_ce_f32")


def adam(param, grad, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8):
    lib = require_gpu()
    n = param.numel()
    assert grad.numel() == n and m.numel() == n and v.numel() == n and param.is_contiguous() and grad.is_contiguous()
    _check(lib.xv_adam_f32(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), n, float(lr_t), float(beta1), float(beta2), float(eps), _stream()),
           "xv_adam_f32")


def ema(moving, batch, decay):
    lib = require_gpu()
    _check(lib.xv_ema_f32(_ptr(moving), _ptr(batch), moving.numel(), float(decay), _stream()), "xv_ema_f32")


def axpy(y, x, a):
    lib = require_gpu()
    assert y.numel() == x.numel() and y.is_contiguous() and x.is_contiguous()
    _check(lib.xv_axpy_f32(_ptr(y), _ptr(x), float(a), y.numel(), _stream()), "xv_axpy_f32")


def sumsq(x, out):
    lib = require_gpu()
    assert x.is_contiguous()
    ws = _ws(lib.xv_sumsq_workspace_bytes(x.numel()), x.device)
    _check(lib.xv_sumsq_f32(_ptr(x), x.numel(), _ptr(out), _ptr(ws), _stream()), "xv_sumsq_f32")


def minibatch_layout(B, T, gap, rows, device):
    """(row_start[B] int32, row_len[B] int32, row_valid[rows] uint8) of a minibatch of B chunks of T frames, generated on the device."""
    import torch
    lib = require_gpu()
    rs = torch.empty(B, dtype=torch.int32, device=device)
    rl = torch.empty(B, dtype=torch.int32, device=device)
    rv = torch.empty(rows, dtype=torch.uint8, device=device)
    _check(lib.xv_minibatch_layout(int(B), int(T), int(gap), int(rows), _ptr(rs), _ptr(rl), _ptr(rv), _stream()), "xv_minibatch_layout")
    return rs, rl, rv


def pack_minibatch(src, B, T, F, gap, dst):
    """src: device tensor holding a [B, T, F] minibatch (float16 or float32, contiguous) -> dst[rows, in_dim] float32: the packed
    rows with gaps (chunk b at rows gap + b*(T+gap)), everything else zero."""
    import torch
    lib = require_gpu()
    assert src.is_cuda and src.is_contiguous() and src.dtype in (torch.float16, torch.float32) and src.numel() >= B * T * F
    _f32(dst, "dst"); assert dst.dim() == 2 and dst.is_contiguous()
    _check(lib.xv_pack_minibatch_f32(_ptr(src), 1 if src.dtype == torch.float16 else 0, int(B), int(T), int(F), int(gap), dst.shape[1],
                                     _ptr(dst), dst.shape[0], _stream()), "xv_pack_minibatch_f32")


def dropout(x, seed, keep_prob, rows=None):
    """In-place tf.nn.dropout on x[R, C] with the stateless mask of include/xvector_hip.h (same call = backward)."""
    lib = require_gpu()
    _rows2d(x, "x")
    R = x.shape[0] if rows is None else int(rows)
    _check(lib.xv_dropout_f32(_ptr(x), x.stride(0), R, x.shape[1], int(seed) & 0xFFFFFFFFFFFFFFFF, float(keep_prob), _stream()),
           "xv_dropout_f32")


def dropout_mask_reference(seed, R, C, keep_prob):
    """NumPy restatement of the kernel's mask (bool [R, C]); used by tests and to hand the oracle the same mask."""
    import numpy as np
    idx = np.arange(1, R * C + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ (idx * np.uint64(0x9E3779B97F4A7C15))
        x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    thr = min(float(np.float32(keep_prob)) * 4294967296.0, 4294967295.0)
    return ((x >> np.uint64(32)).astype(np.int64) < int(np.uint32(thr))).reshape(R, C)


def prelu_backward(dr, z, alpha):
    lib = require_gpu()
    _f32(dr, "dr"); _f32(z, "z"); _f32(alpha, "alpha")
    assert dr.shape == z.shape and dr.stride(0) == z.stride(0) and alpha.numel() == dr.shape[1]
    _check(lib.xv_prelu_backward_f32(_ptr(dr), _ptr(z), dr.stride(0), dr.shape[0], dr.shape[1], _ptr(alpha), _stream()),
           "xv_prelu_backward_f32")


def cmn_sliding_scatter(x, utt_start, utt_len, n_utts, max_len, cmn_window, center, min_window, dst_row, y):
    """Sliding-window CMN of the utterances in x[sum T, F] scattered to rows dst_row[t] of y (see include/xvector_hip.h)."""
    import torch
    lib = require_gpu()
    _f32(x, "x")
    _rows2d(y, "y"); assert y.shape[1] >= x.shape[1]
    i32 = torch.int32
    _check(lib.xv_cmn_sliding_scatter_f32(_ptr(x), x.stride(0), x.shape[1], _dev(utt_start, i32, "utt_start", n_utts),
                                          _dev(utt_len, i32, "utt_len", n_utts), int(n_utts), int(max_len), int(cmn_window),
                                          1 if center else 0, int(min_window), _dev(dst_row, i32, "dst_row", x.shape[0]), _ptr(y),
                                          y.stride(0), _stream()), "xv_cmn_sliding_scatter_f32")


def cmn_sliding_gather(x, utt_start, utt_len, voiced_count, voiced_row, chunk_utt, chunk_first, chunk_len, chunk_row, max_chunk_len,
                       cmn_window, center, min_window, y):
    """xv_cmn_sliding_gather_f32: raw rows x[x_rows, F] (cuda float32, row stride >= F) -> rows of y[y_rows, >= F] (cuda float32): chunk
    c = chunk_len[c] voiced frames of utterance chunk_utt[c] from voiced frame chunk_first[c] on, normalised (sliding-window CMN over
    the RAW frames) and written to rows chunk_row[c] .. of y.  All tables cuda int32; voiced_count / voiced_row are vad_compact's, or
    both None when every frame is voiced.  The kernel checks every row against x, the voiced counts and y (see include/xvector_hip.h)."""
    import torch
    lib = require_gpu()
    _f32_rows(x, "x"); _f32_rows(y, "y")
    i32 = torch.int32
    n_utts, n_chunks = utt_start.numel(), chunk_utt.numel()
    assert (voiced_count is None) == (voiced_row is None), "voiced_count and voiced_row go together"
    _check(lib.xv_cmn_sliding_gather_f32(_ptr(x), x.stride(0), x.shape[1], x.shape[0], _dev(utt_start, i32, "utt_start"),
                                         _dev(utt_len, i32, "utt_len", n_utts), n_utts,
                                         None if voiced_count is None else _dev(voiced_count, i32, "voiced_count", n_utts),
                                         None if voiced_row is None else _dev(voiced_row, i32, "voiced_row", x.shape[0]),
                                         _dev(chunk_utt, i32, "chunk_utt"), _dev(chunk_first, i32, "chunk_first", n_chunks),
                                         _dev(chunk_len, i32, "chunk_len", n_chunks), _dev(chunk_row, i32, "chunk_row", n_chunks),
                                         n_chunks, int(max_chunk_len), int(cmn_window), 1 if center else 0, int(min_window), _ptr(y),
                                         y.stride(0), y.shape[0], _stream()), "xv_cmn_sliding_gather_f32")


def vad_compact(vad, utt_start, utt_len):
    """xv_vad_compact_i32: vad[n_frames] cuda float32 (non-zero = voiced), utt_start / utt_len cuda int32 -> (voiced_count[n_utts],
    voiced_row[n_frames]) cuda int32; voiced_row[utt_start[u] + j] is the frame inside u of its j-th voiced frame."""
    import torch
    lib = require_gpu()
    _f32(vad, "vad")
    starts, lens = _dev(utt_start, torch.int32, "utt_start"), _dev(utt_len, torch.int32, "utt_len")
    n_utts, n_frames = utt_start.numel(), vad.numel()
    assert vad.dim() == 1 and utt_len.numel() == n_utts
    count = torch.zeros(n_utts, dtype=torch.int32, device=vad.device)
    rows = torch.full((max(n_frames, 1),), -1, dtype=torch.int32, device=vad.device)
    _check(lib.xv_vad_compact_i32(_ptr(vad), starts, lens, n_utts, n_frames, _ptr(count), _ptr(rows), _stream()), "xv_vad_compact_i32")
    return count, rows


def vad_segments_workspace_bytes(n_frames):
    """xv_vad_segments_workspace_bytes: what ``vad_segments`` needs for a buffer of ``n_frames`` decisions (host function)."""
    return int(load().xv_vad_segments_workspace_bytes(int(n_frames)))


def vad_segments_capacity(T, max_gap, min_len, max_len):
    """xv_vad_segments_capacity: the most segments an utterance of ``T`` frames can have (host function); ValueError for a negative
    ``T`` or parameters outside the rule's ranges."""
    cap = int(load().xv_vad_segments_capacity(int(T), int(max_gap), int(min_len), int(max_len)))
    if cap < 0:
        raise ValueError("vad_segments_capacity: T = %d, max_gap = %d, min_len = %d, max_len = %d are outside the rule's ranges"
                         % (T, max_gap, min_len, max_len))
    return cap


def vad_segments(vad, utt_start, utt_len, max_gap, min_len, pad, max_len, seg_off, seg_cap, seg_count, seg_first, seg_len,
                 workspace=None):
    """xv_vad_segments_i32: vad[n_frames] cuda float32 (non-zero = voiced), utt_start / utt_len / seg_off / seg_cap cuda int32, one
    entry per utterance -> seg_count[n_utts] (the full count), and segment i of utterance u in seg_first / seg_len[seg_off[u] + i]
    (cuda int32, equally long: the slots) while i < seg_cap[u].  The rule: include/xvector_hip.h.  Entries no segment names keep
    their contents.  ``workspace``: a cuda uint8 tensor of at least ``vad_segments_workspace_bytes`` bytes (None: made here)."""
    import torch
    lib = require_gpu()
    _f32(vad, "vad")
    i32, n_utts, n_frames, n_slots = torch.int32, utt_start.numel(), vad.numel(), seg_first.numel()
    assert vad.dim() == 1 and seg_len.numel() == n_slots
    need = vad_segments_workspace_bytes(n_frames)
    if workspace is None:
        workspace = _ws(need, vad.device)
    _check(lib.xv_vad_segments_i32(_ptr(vad), _dev(utt_start, i32, "utt_start"), _dev(utt_len, i32, "utt_len", n_utts), n_utts,
                                   n_frames, int(max_gap), int(min_len), int(pad), int(max_len), _dev(seg_off, i32, "seg_off", n_utts),
                                   _dev(seg_cap, i32, "seg_cap", n_utts), n_slots, _dev(seg_count, i32, "seg_count", n_utts),
                                   _dev(seg_first, i32, "seg_first"), _dev(seg_len, i32, "seg_len"),
                                   _dev(workspace, torch.uint8, "workspace", need), _nbytes(workspace), _stream()), "xv_vad_segments_i32")
    return seg_count, seg_first, seg_len


def voiced_rank(vad, utt_start, utt_len, n_frames, rank=None, count=None):
    """xv_voiced_rank_i32: vad[>= n_frames] cuda float32 (non-zero = voiced; None: every frame is voiced), utt_start / utt_len cuda
    int32 -> (rank[n_frames], voiced_count[n_utts]) cuda int32: rank[utt_start[u] + t] = voiced frames of u before t, -1 for an
    unvoiced frame.  Entries of ``rank`` outside the utterances' spans are not written (a fresh ``rank`` is uninitialised there)."""
    import torch
    lib = require_gpu()
    i32, n_utts, n_frames = torch.int32, utt_start.numel(), int(n_frames)
    assert n_frames >= 0 and utt_len.numel() == n_utts
    if vad is not None:
        _f32(vad, "vad")
        assert vad.dim() == 1 and vad.numel() >= n_frames, "vad must hold at least %d decisions" % n_frames
    dev = utt_start.device
    if rank is None:
        rank = torch.empty(max(n_frames, 1), dtype=i32, device=dev)
    if count is None:
        count = torch.empty(max(n_utts, 1), dtype=i32, device=dev)
    _check(lib.xv_voiced_rank_i32(_ptr(vad), _dev(utt_start, i32, "utt_start"), _dev(utt_len, i32, "utt_len"), n_utts, n_frames,
                                  _dev(rank, i32, "rank", n_frames), _dev(count, i32, "count", n_utts), _stream()), "xv_voiced_rank_i32")
    return rank, count[:n_utts]


def chunk_row_plan(rank, utt_start, utt_len, chunk_size, chunks_kept, first_chunk, n_frames, b0, b1, row_start, dst_row=None):
    """xv_chunk_row_plan_i32: ``rank`` of voiced_rank + the per-utterance chunk tables (cuda int32, one entry per utterance of
    utt_start) -> dst_row[n_frames] cuda int32, the row of the packed batch of chunks [b0, b1) (chunk c at row_start[c - b0]) each
    feature row goes to, or -1.  Only the rows of the listed utterances are written."""
    import torch
    lib = require_gpu()
    i32, n_utts, n_frames = torch.int32, utt_start.numel(), int(n_frames)
    assert n_frames >= 0 and int(b1) >= int(b0)
    if dst_row is None:
        dst_row = torch.empty(max(n_frames, 1), dtype=i32, device=rank.device)
    _check(lib.xv_chunk_row_plan_i32(_dev(rank, i32, "rank", n_frames), _dev(utt_start, i32, "utt_start"),
                                     _dev(utt_len, i32, "utt_len", n_utts), _dev(chunk_size, i32, "chunk_size", n_utts),
                                     _dev(chunks_kept, i32, "chunks_kept", n_utts), _dev(first_chunk, i32, "first_chunk", n_utts),
                                     n_utts, n_frames, int(b0), int(b1), _dev(row_start, i32, "row_start", int(b1) - int(b0)),
                                     _dev(dst_row, i32, "dst_row", n_frames), _stream()), "xv_chunk_row_plan_i32")
    return dst_row


def check_chunk_table(table, voiced_counts, feat_dim, y_elems):
    """The chunk table (host arrays chunk_utt, chunk_first, chunk_len, chunk_dst) against host copies of the voiced counts and the
    size of the destination: ValueError names the first chunk that would leave its utterance or the buffer.  Pure NumPy."""
    import numpy as np
    cu, cf, cl, cd = (np.asarray(a, np.int64).reshape(-1) for a in table)
    counts = np.asarray(voiced_counts, np.int64).reshape(-1)
    if not (len(cu) == len(cf) == len(cl) == len(cd)):
        raise ValueError("chunk table: columns of different lengths")
    bad = (cu < 0) | (cu >= len(counts))
    if not bad.any():
        bad = (cf < 0) | (cl <= 0) | (cf + cl > counts[cu]) | (cd < 0) | (cd + cl * int(feat_dim) > int(y_elems))
    if bad.any():
        c = int(np.flatnonzero(bad)[0])
        n = int(counts[cu[c]]) if 0 <= cu[c] < len(counts) else -1
        raise ValueError("chunk %d of the table (utterance %d, voiced frames [%d, %d), %d halves from %d) does not fit: the utterance "
                         "has %d voiced frames, the destination %d halves" % (c, cu[c], cf[c], cf[c] + cl[c], cl[c] * int(feat_dim),
                                                                             cd[c], n, int(y_elems)))
    return cu.astype(np.int32), cf.astype(np.int32), cl.astype(np.int32), cd


def egs_chunks(x, utt_start, utt_len, voiced_count, voiced_row, table, voiced_counts_host, cmn_window, center, min_window, y):
    """xv_egs_chunks_f16: raw rows x[n_frames, F] (cuda float32, row stride >= F) -> float16 chunks in the flat cuda float16 tensor y.
    ``table`` = host arrays (chunk_utt, chunk_first, chunk_len, chunk_dst); it is checked against ``voiced_counts_host`` (a host copy
    of voiced_count) and y.numel() first: ValueError before anything is launched."""
    import numpy as np
    import torch
    lib = require_gpu()
    _f32_rows(x, "x"); _dev(y, torch.float16, "y")
    for t, name in ((utt_start, "utt_start"), (utt_len, "utt_len"), (voiced_count, "voiced_count"), (voiced_row, "voiced_row")):
        _dev(t, torch.int32, name)
    n_utts = utt_start.numel()
    assert utt_len.numel() == n_utts and voiced_count.numel() == n_utts and voiced_row.numel() >= x.shape[0]
    assert len(voiced_counts_host) == n_utts
    cu, cf, cl, cd = check_chunk_table(table, voiced_counts_host, x.shape[1], y.numel())
    if len(cu) == 0:
        return
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(x.device) for a in (cu, cf, cl, cd)]
    _check(lib.xv_egs_chunks_f16(_ptr(x), x.stride(0), x.shape[1], x.shape[0], _ptr(utt_start), _ptr(utt_len), n_utts, _ptr(voiced_count),
                                 _ptr(voiced_row), _ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), len(cu), int(cl.max()),
                                 int(cmn_window), 1 if center else 0, int(min_window), _ptr(y), y.numel(), _stream()),
           "xv_egs_chunks_f16")


def backend_prepare(x, out, side, num_utts=None, mean=None, lda=None, lda_offset=None, length_norm=True, plda_transform=None,
                    plda_mean=None, plda_psi=None, r=None):
    """Operand rows of the scorers from raw vectors x[N, D] (see include/xvector_hip.h): mean subtraction, LDA, length norm,
    PLDA transform and length norm, packed for ``side`` into out[N, Kpad] (zeros past K); r[N] the per-row constant.  x and lda may
    be slices of wider buffers (dense rows; the row stride is passed as ldx / ld_lda)."""
    import torch
    lib = require_gpu()
    _f32_rows(x, "x"); _f32(out, "out")
    n_rows, dim_in = x.shape
    dim = lda.shape[0] if lda is not None else dim_in
    assert out.shape[0] >= n_rows and out.shape[1] == out.stride(0)
    for t, shape in ((mean, (dim_in,)), (lda_offset, (dim,)), (plda_transform, (dim, dim)), (plda_mean, (dim,)), (plda_psi, (dim,)),
                     (r, (n_rows,))):
        if t is not None:
            assert tuple(_f32(t, "a parameter vector").shape) == shape, shape
    if lda is not None:
        _f32_rows(lda, "lda"); assert lda.shape[1] == dim_in
    if num_utts is not None:
        _dev(num_utts, torch.int32, "num_utts", n_rows)
    _check(lib.xv_backend_prepare_f32(_ptr(x), x.stride(0), n_rows, dim_in, _ptr(num_utts), _ptr(mean), _ptr(lda),
                                      lda.stride(0) if lda is not None else 0, _ptr(lda_offset), dim, 1 if length_norm else 0,
                                      _ptr(plda_transform), _ptr(plda_mean), _ptr(plda_psi), int(side), _ptr(out), out.stride(0),
                                      _ptr(r), _stream()), "xv_backend_prepare_f32")


def score_matrix(e, t, r, out):
    """out[Ne, Nt] = e[Ne, Kpad] t[Nt, Kpad]^T + r[Ne] (r may be None), fixed summation order (k ascending).  e and t may be
    slices of wider buffers with one common row stride, passed as ldk (a multiple of 4, bases 16-byte aligned)."""
    lib = require_gpu()
    _f32_rows(e, "e"); _f32_rows(t, "t"); _f32(out, "out")
    assert e.shape[1] == t.shape[1] and e.stride(0) == t.stride(0) and out.shape[0] >= e.shape[0] and out.shape[1] >= t.shape[0]
    assert r is None or _f32(r, "r").numel() >= e.shape[0]
    _check(lib.xv_score_matrix_f32(_ptr(e), _ptr(t), e.stride(0), e.shape[1], e.shape[0], t.shape[0], _ptr(r), _ptr(out), out.stride(0),
                                   _stream()), "xv_score_matrix_f32")


def score_blocks(e, t, r, grp_row0, grp_score0, max_n, out, status):
    """Block-diagonal self-scoring of ragged groups of rows (xv_score_blocks_f32; see include/xvector_hip.h): group g is rows
    [grp_row0[g], grp_row0[g + 1]) of e, t and r, its n_g x n_g matrix goes to out + grp_score0[g] with row stride
    (n_g + 3) & ~3, each cell with the bits score_matrix gives those two rows.  grp_row0: int32 [G + 1], grp_score0: int64 [G],
    out: float32 1-D, status: int32 [1] (zeroed by the caller, 1 after a group out of contract was skipped), all on the device."""
    import torch
    lib = require_gpu()
    _f32_rows(e, "e"); _f32_rows(t, "t"); _f32(out, "out")
    assert e.shape == t.shape and e.stride(0) == t.stride(0)
    assert r is None or _f32(r, "r").numel() >= e.shape[0]
    n_groups = grp_score0.numel()
    _check(lib.xv_score_blocks_f32(_ptr(e), _ptr(t), e.stride(0), e.shape[1], e.shape[0], _ptr(r),
                                   _dev(grp_row0, torch.int32, "grp_row0", n_groups + 1), _dev(grp_score0, torch.int64, "grp_score0"),
                                   n_groups, int(max_n), _ptr(out), out.numel(), _dev(status, torch.int32, "status", 1), _stream()),
           "xv_score_blocks_f32")


def score_pairs(e, t, r, e_idx, t_idx, out):
    """out[i] = e[e_idx[i]] . t[t_idx[i]] + r[e_idx[i]]: bit-identical to the cell of score_matrix.  The kernel reads the rows the
    indices name, so their range is checked here first.  e and t may be slices of wider buffers, as for score_matrix."""
    import torch
    lib = require_gpu()
    _f32_rows(e, "e"); _f32_rows(t, "t")
    assert e.shape[1] == t.shape[1] and e.stride(0) == t.stride(0)
    _dev(e_idx, torch.int32, "e_idx"); _dev(t_idx, torch.int32, "t_idx")
    m = e_idx.numel()
    assert t_idx.numel() == m and _f32(out, "out").numel() >= m
    assert r is None or _f32(r, "r").numel() >= e.shape[0]
    if m:
        lo = torch.stack([e_idx.min(), t_idx.min(), e_idx.max() - e.shape[0], t_idx.max() - t.shape[0]]).cpu().tolist()
        if lo[0] < 0 or lo[1] < 0 or lo[2] >= 0 or lo[3] >= 0:
            raise XvectorHipError("score_pairs: trial index out of range")
    _check(lib.xv_score_pairs_f32(_ptr(e), _ptr(t), e.stride(0), e.shape[1], _ptr(e_idx), _ptr(t_idx), m, _ptr(r), _ptr(out), _stream()),
           "xv_score_pairs_f32")


def topk_row_stats(scores, top_n, mean, std):
    """mean[i], std[i] = mean and population std of the top_n largest values of row i of scores[R, C] (exact selection, fp64 sums;
    see include/xvector_hip.h).  scores may be a row slice of a wider buffer: its row stride is passed as ld."""
    lib = require_gpu()
    n_rows, n_cols = _rows2d(scores, "scores").shape
    assert _f32(mean, "mean").numel() >= n_rows and _f32(std, "std").numel() >= n_rows
    _check(lib.xv_topk_row_stats_f32(_ptr(scores), scores.stride(0), n_rows, n_cols, int(top_n), _ptr(mean), _ptr(std), _stream()),
           "xv_topk_row_stats_f32")


def moment_stats_workspace_bytes(n_rows, dim):
    return int(load().xv_moment_stats_workspace_bytes(int(n_rows), int(dim)))


def moment_stats(x, sum, outer, dim=None, workspace=None):
    """sum[j] = sum_i x[i, j], outer[j, k] = sum_i x[i, j] x[i, k] over the rows of x[N, >= dim] in fp64 on the f64 MFMA, in a
    fixed order (see include/xvector_hip.h).  x may be a slice of a wider buffer (its row stride is passed as ldx; dim None: all
    of its columns); sum: float64 [>= dim]; outer: float64 [>= dim, ld] (its row stride is passed as ld_outer).  workspace: a
    device buffer of moment_stats_workspace_bytes(N, dim) bytes (None: allocated here)."""
    import torch
    lib = require_gpu()
    _rows2d(x, "x")
    n_rows = x.shape[0]
    dim = x.shape[1] if dim is None else int(dim)
    assert dim <= x.shape[1]
    assert outer.is_cuda and outer.dtype == torch.float64 and outer.dim() == 2 and outer.stride(1) == 1
    assert outer.shape[0] >= dim and outer.shape[1] >= dim
    if workspace is None:
        workspace = _ws(lib.xv_moment_stats_workspace_bytes(n_rows, dim), x.device)
    _check(lib.xv_moment_stats_f64(_ptr(x), x.stride(0), n_rows, dim, _dev(sum, torch.float64, "sum", dim), _ptr(outer), outer.stride(0),
                                   _ptr(workspace), _nbytes(workspace), _stream()), "xv_moment_stats_f64")


def ahc_average_workspace_bytes(n):
    return int(load().xv_ahc_average_workspace_bytes(int(n)))


def ahc_average(scores, threshold, min_clusters, merge_a, merge_b, merge_score, n_merges, labels, workspace=None):
    """Average-linkage agglomerative clustering of the n items of scores[n, n] (xv_ahc_average_f64; see include/xvector_hip.h):
    only the strict upper triangle is read.  scores may be a slice of a wider buffer (its row stride is passed as ld, a multiple
    of 4).  merge_a, merge_b: int32 [>= n - 1]; merge_score: float64 [>= n - 1]; n_merges: int32 [1]; labels: int32 [>= n], all
    on the device and written there: nothing is read back and the stream is not synchronised.  workspace: a device buffer of
    ahc_average_workspace_bytes(n) bytes (None: allocated here)."""
    import math
    import torch
    lib = require_gpu()
    _rows2d(scores, "scores")
    n = scores.shape[0]
    assert scores.shape[1] == n and 1 <= n <= AHC_MAX_N, "scores must be [n, n], 1 <= n <= %d" % AHC_MAX_N
    assert scores.stride(0) >= n and scores.stride(0) % 4 == 0 and scores.data_ptr() % 16 == 0
    assert 1 <= int(min_clusters) <= n and not math.isnan(float(threshold))
    need = lib.xv_ahc_average_workspace_bytes(n)
    if workspace is None:
        workspace = _ws(need, scores.device)
    assert workspace.is_cuda and _nbytes(workspace) >= need, "ahc workspace too small"
    i32 = torch.int32
    _check(lib.xv_ahc_average_f64(_ptr(scores), scores.stride(0), n, float(threshold), int(min_clusters),
                                  _dev(merge_a, i32, "merge_a", n - 1), _dev(merge_b, i32, "merge_b", n - 1),
                                  _dev(merge_score, torch.float64, "merge_score", n - 1), _dev(n_merges, i32, "n_merges", 1),
                                  _dev(labels, i32, "labels", n), _ptr(workspace), _nbytes(workspace), _stream()), "xv_ahc_average_f64")


def ahc_average_batch_workspace_bytes(n):
    return int(load().xv_ahc_average_batch_workspace_bytes(int(n)))


def ahc_average_batch(scores, grp_row0, grp_score0, grp_ws0, threshold, min_clusters, max_n, merge_a, merge_b, merge_score, n_merges,
                      labels, status, workspace):
    """G independent average-linkage problems in one launch, one workgroup each (xv_ahc_average_batch_f64; see
    include/xvector_hip.h).  scores: float32 1-D, the packed blocks score_blocks writes; grp_row0: int32 [G + 1]; grp_score0,
    grp_ws0: int64 [G] (element offsets into scores, byte offsets into workspace); threshold: float64 [G]; min_clusters: int32 [G].
    merge_a, merge_b: int32 [>= n_rows]; merge_score: float64 [>= n_rows]; n_merges: int32 [>= G]; labels: int32 [>= n_rows] with
    n_rows = len(labels); status: int32 [1], zeroed by the caller.  Everything is on the device and written there: nothing is read
    back and the stream is not synchronised.  Put large groups first: workgroups tend to start in group order (only speed depends on it)."""
    import torch
    lib = require_gpu()
    _f32(scores, "scores")
    n_groups = grp_score0.numel()
    n_rows = labels.numel()
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    assert workspace.is_cuda and workspace.is_contiguous()
    _check(lib.xv_ahc_average_batch_f64(_ptr(scores), scores.numel(), _dev(grp_row0, i32, "grp_row0", n_groups + 1),
                                        _dev(grp_score0, i64, "grp_score0"), _dev(grp_ws0, i64, "grp_ws0", n_groups),
                                        _dev(threshold, f64, "threshold", n_groups), _dev(min_clusters, i32, "min_clusters", n_groups),
                                        n_groups, int(max_n), n_rows, _dev(merge_a, i32, "merge_a", n_rows),
                                        _dev(merge_b, i32, "merge_b", n_rows), _dev(merge_score, f64, "merge_score", n_rows),
                                        _dev(n_merges, i32, "n_merges", n_groups), _dev(labels, i32, "labels"),
                                        _dev(status, i32, "status", 1), _ptr(workspace), _nbytes(workspace), _stream()),
           "xv_ahc_average_batch_f64")


def pca_plda_groups_workspace_bytes(n_groups, dim):
    return int(load().xv_pca_plda_groups_workspace_bytes(int(n_groups), int(dim)))


def pca_plda_groups(y, grp_row0, dim, target_energy, mean, within, between, transform, psi, grp_dim, grp_info, eigvals, pca, grp_psi,
                    grp_map, grp_off, status, workspace=None):
    """Per-group PCA and the PLDA projected into it (xv_pca_plda_groups_f64; see include/xvector_hip.h).  y: float32 rows
    [n_rows, >= dim] (its row stride is passed as ldy); grp_row0: int32 [G + 1]; the model mean, psi: float64 [dim], within,
    between, transform: float64 [dim, dim].  Outputs, all on the device: grp_dim, grp_info: int32 [G]; eigvals, grp_psi, grp_off:
    float64 [G, dim]; pca (or None), grp_map: float64 [G, dim, dim]; status: int32 [1], zeroed by the caller.  Nothing is read
    back and the stream is not synchronised.  workspace: pca_plda_groups_workspace_bytes(G, dim) bytes (None: allocated here)."""
    import torch
    lib = require_gpu()
    _rows2d(y, "y")
    i32, f64 = torch.int32, torch.float64
    G = grp_dim.numel()
    dim = int(dim)
    assert y.shape[1] >= dim
    need = lib.xv_pca_plda_groups_workspace_bytes(G, dim)
    if workspace is None:
        workspace = _ws(need, y.device)
    assert workspace.is_cuda and workspace.is_contiguous()
    _check(lib.xv_pca_plda_groups_f64(_ptr(y), y.stride(0), y.shape[0], _dev(grp_row0, i32, "grp_row0", G + 1), G, dim,
                                      float(target_energy), _dev(mean, f64, "mean", dim), _dev(within, f64, "within", dim * dim),
                                      _dev(between, f64, "between", dim * dim), _dev(transform, f64, "transform", dim * dim),
                                      _dev(psi, f64, "psi", dim), _dev(grp_dim, i32, "grp_dim"), _dev(grp_info, i32, "grp_info", G),
                                      _dev(eigvals, f64, "eigvals", G * dim), None if pca is None else _dev(pca, f64, "pca", G * dim * dim),
                                      _dev(grp_psi, f64, "grp_psi", G * dim), _dev(grp_map, f64, "grp_map", G * dim * dim),
                                      _dev(grp_off, f64, "grp_off", G * dim), _dev(status, i32, "status", 1), _ptr(workspace),
                                      _nbytes(workspace), _stream()), "xv_pca_plda_groups_f64")


def backend_prepare_groups(y, grp_row0, max_n, dim, grp_dim, grp_psi, grp_map, grp_off, side, out, r, status):
    """The grouped twin of backend_prepare's PLDA stage (xv_backend_prepare_groups_f32; see include/xvector_hip.h): every row of
    y [n_rows, >= dim] through its group's z = M_g y + c_g, the PLDA length norm with psi_g and p_g, and the operand row of
    ``side`` (SIDE_ENROL | SIDE_TEST) in out[n_rows, ldo] with exact zeros past 2 p_g; r: float32 [n_rows] or None."""
    import torch
    lib = require_gpu()
    _rows2d(y, "y"); _f32_rows(out, "out")
    i32, f64 = torch.int32, torch.float64
    G = grp_dim.numel()
    dim = int(dim)
    n_rows = y.shape[0]
    assert y.shape[1] >= dim and out.shape[0] >= n_rows and out.shape[1] == out.stride(0)
    assert r is None or _f32(r, "r").numel() >= n_rows
    _check(lib.xv_backend_prepare_groups_f32(_ptr(y), y.stride(0), n_rows, _dev(grp_row0, i32, "grp_row0", G + 1), G, int(max_n), dim,
                                             _dev(grp_dim, i32, "grp_dim"), _dev(grp_psi, f64, "grp_psi", G * dim),
                                             _dev(grp_map, f64, "grp_map", G * dim * dim), _dev(grp_off, f64, "grp_off", G * dim),
                                             int(side), _ptr(out), out.stride(0), _ptr(r), _dev(status, i32, "status", 1), _stream()),
           "xv_backend_prepare_groups_f32")


def vbx_groups_workspace_bytes(n_rows, n_groups, dim, max_spk):
    return int(load().xv_vbx_groups_workspace_bytes(int(n_rows), int(n_groups), int(dim), int(max_spk)))


def vbx_groups(y, grp_row0, dim, row_of_t, init_label, grp_spk, max_spk, mean, transform, psi, fa, fb, loop_prob, init_smoothing,
               max_iters, epsilon, labels, gamma, pi, elbo, grp_iters, grp_info, status, workspace=None):
    """VBx resegmentation of every group's rows (xv_vbx_groups_f64; see include/xvector_hip.h for the rule).  y: float32 rows
    [n_rows, >= dim] (its row stride is passed as ldy); grp_row0: int32 [G + 1]; row_of_t: int32 [n_rows] or None (the identity);
    init_label: int32 [n_rows]; grp_spk: int32 [G]; the model mean, psi: float64 [dim], transform: float64 [dim, dim].  Outputs,
    all on the device: labels int32 [n_rows]; gamma float64 [n_rows, max_spk] or None; pi float64 [G, max_spk]; elbo float64
    [G, max_iters]; grp_iters, grp_info: int32 [G]; status: int32 [1], zeroed by the caller.  Nothing is read back and the stream
    is not synchronised.  workspace: vbx_groups_workspace_bytes(n_rows, G, dim, max_spk) bytes (None: allocated here)."""
    import torch
    lib = require_gpu()
    _rows2d(y, "y")
    i32, f64 = torch.int32, torch.float64
    G = grp_spk.numel()
    dim, max_spk, max_iters = int(dim), int(max_spk), int(max_iters)
    n_rows = y.shape[0]
    assert y.shape[1] >= dim
    if workspace is None:
        workspace = _ws(lib.xv_vbx_groups_workspace_bytes(n_rows, G, dim, max_spk), y.device)
    assert workspace.is_cuda and workspace.is_contiguous()
    _check(lib.xv_vbx_groups_f64(_ptr(y), y.stride(0), n_rows, _dev(grp_row0, i32, "grp_row0", G + 1), G, dim,
                                 None if row_of_t is None else _dev(row_of_t, i32, "row_of_t", n_rows),
                                 _dev(init_label, i32, "init_label", n_rows), _dev(grp_spk, i32, "grp_spk"), max_spk,
                                 _dev(mean, f64, "mean", dim), _dev(transform, f64, "transform", dim * dim), _dev(psi, f64, "psi", dim),
                                 float(fa), float(fb), float(loop_prob), float(init_smoothing), max_iters, float(epsilon),
                                 _dev(labels, i32, "labels", n_rows),
                                 None if gamma is None else _dev(gamma, f64, "gamma", n_rows * max(max_spk, 0)),
                                 _dev(pi, f64, "pi", G * max(max_spk, 0)), _dev(elbo, f64, "elbo", G * max(max_iters, 0)),
                                 _dev(grp_iters, i32, "grp_iters", G), _dev(grp_info, i32, "grp_info", G),
                                 _dev(status, i32, "status", 1), _ptr(workspace), _nbytes(workspace), _stream()), "xv_vbx_groups_f64")


def mfcc(samples, utt_offset, utt_samples, utt_row0, utt_key, total_rows, tables, opts, feats, logmel=None):
    """MFCC rows of a window of utterances (xv_mfcc_f32; see include/xvector_hip.h).  samples: int16 or float32 (1-D, device);
    utt_*: int64 device tensors (utt_key as int64 bit patterns); tables: the device tables of ``mfcc.MfccTables``
    (window, mel_first, mel_len, mel_w, lifter_dct, twiddle); opts: ``mfcc.MfccOptions``.  feats [rows, ld] float32 (ld >=
    num_ceps), logmel [rows, ld] or None."""
    import torch
    lib = require_gpu()
    assert samples.is_cuda and samples.dim() == 1 and samples.dtype in (torch.int16, torch.float32)
    for t, name in ((utt_offset, "utt_offset"), (utt_samples, "utt_samples"), (utt_row0, "utt_row0"), (utt_key, "utt_key")):
        _dev(t, torch.int64, name); assert t.numel() == utt_offset.numel()
    for t in (feats, logmel):
        assert t is None or _rows2d(t, "feats / logmel").shape[0] >= total_rows
    tb = tables
    _check(lib.xv_mfcc_f32(_ptr(samples), 0 if samples.dtype == torch.int16 else 1, _ptr(utt_offset), _ptr(utt_samples),
                           _ptr(utt_row0), _ptr(utt_key), int(utt_offset.numel()), int(total_rows), _ptr(tb["window"]),
                           _ptr(tb["mel_first"]), _ptr(tb["mel_len"]), _ptr(tb["mel_w"]), int(tb["mel_w"].shape[0]),
                           int(tb["mel_w"].shape[1]), _ptr(tb["lifter_dct"]), int(tb["lifter_dct"].shape[0]), _ptr(tb["twiddle"]),
                           opts.frame_length_samples, opts.frame_shift_samples, opts.padded_length, int(opts.snip_edges),
                           float(opts.dither), float(opts.preemphasis_coefficient), int(opts.remove_dc_offset),
                           int(opts.use_energy), int(opts.raw_energy), float(opts.energy_floor), _ptr(feats), feats.stride(0),
                           _ptr(logmel), 0 if logmel is None else logmel.stride(0), _stream()), "xv_mfcc_f32")


def vad_energy(feats, utt_row0, n_frames, vopts, out):
    """compute-vad over ragged utterances (xv_vad_energy_f32): column 0 of feats [rows, ld] (any row stride), utterance u = rows
    utt_row0[u] .. + n_frames[u] (int64 / int32 device tensors); out[rows] float32 receives 0.0 / 1.0."""
    import torch
    lib = require_gpu()
    _rows2d(feats, "feats"); _f32(out, "out")
    assert utt_row0.is_cuda and utt_row0.dtype == torch.int64 and n_frames.is_cuda and n_frames.dtype == torch.int32
    _check(lib.xv_vad_energy_f32(_ptr(feats), feats.stride(0), _ptr(utt_row0), _ptr(n_frames), int(utt_row0.numel()),
                                 float(vopts.vad_energy_threshold), float(vopts.vad_energy_mean_scale),
                                 int(vopts.vad_frames_context), float(vopts.vad_proportion_threshold), _ptr(out), _stream()),
           "xv_vad_energy_f32")


def cm_payload_bytes(rows, cols):
    """Bytes of the CompressedMatrix payload of a rows x cols matrix (xv_cm_payload_bytes; 0 for rows == 0)."""
    return int(load().xv_cm_payload_bytes(int(rows), int(cols)))


def cm_encode(feats, utt_row0, n_frames, n_cols, out_offset, out, status):
    """CompressedMatrix payloads of ragged utterances (xv_cm_encode_f32): utterance u = rows utt_row0[u] .. + n_frames[u] of feats
    [rows, ld] (int64 / int32 device tensors, as vad_energy), columns 0 .. n_cols - 1; its payload goes to the uint8 device buffer
    ``out`` at out_offset[u] (int64, multiples of 16: compress.plan), status[u] (int32) receives 0 or the reason it was refused."""
    import torch
    lib = require_gpu()
    _rows2d(feats, "feats")
    n = int(utt_row0.numel())
    assert 1 <= int(n_cols) <= feats.shape[1] and out.dim() == 1 and out.data_ptr() % 16 == 0
    _check(lib.xv_cm_encode_f32(_ptr(feats), feats.stride(0), _dev(utt_row0, torch.int64, "utt_row0"),
                                _dev(n_frames, torch.int32, "n_frames", n), n, int(n_cols), _dev(out_offset, torch.int64, "out_offset", n),
                                _dev(out, torch.uint8, "out"), _dev(status, torch.int32, "status", n), _stream()), "xv_cm_encode_f32")


def resample_num_output(n, rate_in, rate_out):
    """Outputs of n input samples at rate_in resampled to rate_out (xv_resample_num_output; -1 for rates it refuses)."""
    return int(load().xv_resample_num_output(int(n), int(rate_in), int(rate_out)))


def resample(inp, utt, tab, first, ntaps, w, tiles, out):
    """Rate conversion of ragged utterances (xv_resample_f32; see include/xvector_hip.h).  inp: int16 or float32 (1-D, device);
    utt: HOST int64 [5, U] = (in_offset, in_samples, out_offset, out_samples, table) rows, uploaded here; tab: HOST int64
    [n_tables, 6] descriptors; first / ntaps (int32), w (float32), tiles ([n_tiles, 2] int64): device; out: float32 (1-D, device).
    The host side of the ABI's argument checks lives here: every span must lie inside its buffer, and an out_samples beyond
    what the rates give is refused as XV_ERR_BAD_ARG before anything is launched."""
    import numpy as np
    import torch
    lib = require_gpu()
    assert inp.is_cuda and inp.dim() == 1 and inp.dtype in (torch.int16, torch.float32) and inp.is_contiguous()
    assert utt.dtype == np.int64 and utt.ndim == 2 and utt.shape[0] == 5 and tab.dtype == np.int64 and tab.ndim == 2 and tab.shape[1] == 6
    assert tiles.dim() == 2 and tiles.shape[1] == 2 and out.dim() == 1
    utt, tab = np.ascontiguousarray(utt), np.ascontiguousarray(tab)
    in_off, n_in, out_off, n_out, table = utt
    assert np.all((table >= 0) & (table < len(tab))), "utt: table index out of range"
    assert np.all((in_off >= 0) & (n_in >= 0) & (in_off + n_in <= inp.numel())), "utt: an input span leaves inp"
    assert np.all((out_off >= 0) & (n_out >= 0) & (out_off + n_out <= out.numel())), "utt: an output span leaves out"
    if len(tab) and np.all(tab[:, :3] >= 1):
        assert np.all(tab[:, 3] + tab[:, 1] <= min(first.numel(), ntaps.numel())), "tab: phase tables too short"
        assert np.all(tab[:, 4] + tab[:, 1] * tab[:, 2] <= w.numel()), "tab: weight table too short"
        Ui, Uo = tab[table, 0], tab[table, 1]
        L = n_in * Uo                                              # xv_resample_num_output in units of lcm ticks
        most = np.where(L <= 0, 0, (L - 1) // Ui + 1)
        if np.any(n_out > most):
            u = int(np.flatnonzero(n_out > most)[0])
            raise XvectorHipError("xv_resample_f32 failed (-1): resample: out_samples[%d] = %d exceeds the %d outputs of %d input "
                                  "samples" % (u, n_out[u], most[u], n_in[u]))
    d_utt = torch.from_numpy(utt).to(inp.device)
    _check(lib.xv_resample_f32(_ptr(inp), 0 if inp.dtype == torch.int16 else 1, _ptr(d_utt[0]), _ptr(d_utt[1]), _ptr(d_utt[2]),
                               _ptr(d_utt[3]), _ptr(d_utt[4]), int(utt.shape[1]), tab.ctypes.data_as(ctypes.c_void_p), int(len(tab)),
                               _dev(first, torch.int32, "first"), _dev(ntaps, torch.int32, "ntaps"), _dev(w, torch.float32, "w"),
                               _dev(tiles, torch.int64, "tiles"), int(tiles.shape[0]), _dev(out, torch.float32, "out"), _stream()),
           "xv_resample_f32")


def wave_decode(raw, utt, tiles, out, sample_format):
    """Coded audio to samples (xv_wave_decode; see include/xvector_hip.h).  raw: uint8 (1-D, device), the data regions of the
    files; utt: HOST int64 [U, 8] descriptors (RAW_OFF, N, STRIDE, CH_OFF, CODING, OUT_OFF, 0, 0), uploaded here; tiles: [n_tiles,
    2] int64 (device); out: int16 (sample_format 0) or float32 (1), 1-D, device.  The host side of the ABI's argument checks
    lives here, as in ``resample``: every span must lie inside raw and out, CODING and STRIDE must be in range and the channel
    inside its frame, else the call is refused as XV_ERR_BAD_ARG before anything is launched."""
    import numpy as np
    import torch
    lib = require_gpu()
    assert raw.is_cuda and raw.dim() == 1 and raw.dtype == torch.uint8 and raw.is_contiguous()
    assert out.is_cuda and out.dim() == 1 and out.is_contiguous() and sample_format in (0, 1)
    assert out.dtype == (torch.int16 if sample_format == 0 else torch.float32)
    assert isinstance(utt, np.ndarray) and utt.dtype == np.int64 and utt.ndim == 2 and utt.shape[1] == 8
    assert tiles.dim() == 2 and tiles.shape[1] == 2
    utt = np.ascontiguousarray(utt)
    raw_off, n, stride, ch_off, coding, out_off = (utt[:, f] for f in range(6))

    def refuse(bad, what):
        if np.any(bad):
            u = int(np.flatnonzero(bad)[0])
            raise XvectorHipError("xv_wave_decode failed (-1): wave_decode: utterance %d: %s (descriptor %s)" % (u, what, utt[u].tolist()))

    refuse((coding < 0) | (coding > 3), "CODING outside 0 .. 3")
    refuse((stride != 1) & (stride != 2) & (stride != 4), "STRIDE is not 1, 2 or 4")
    refuse((ch_off < 0) | (ch_off + np.where(coding < 2, 2, 1) > stride), "CH_OFF + width exceeds STRIDE")
    refuse(n < 0, "a negative sample count")
    refuse((raw_off < 0) | (n > (raw.numel() - raw_off) // np.maximum(stride, 1)), "the span leaves raw")
    refuse((out_off < 0) | (n > out.numel() - out_off), "the span leaves out")
    refuse((utt[:, 6] != 0) | (utt[:, 7] != 0), "a reserved field is not zero")
    d_utt = torch.from_numpy(utt).to(raw.device)
    _check(lib.xv_wave_decode(_ptr(raw), int(raw.numel()), _ptr(d_utt), int(utt.shape[0]), _dev(tiles, torch.int64, "tiles"),
                              int(tiles.shape[0]), _ptr(out), int(sample_format), _stream()), "xv_wave_decode")


def augment_power(sig, segments, tiles, tile_sumsq):
    """wav-reverberate, step 1 (xv_augment_power_f64): fp64 sums of squares of int16 segments [S, 4] = (off, len, tile0,
    ntiles), per tile [T, 2] = (segment, first sample)."""
    import torch
    lib = require_gpu()
    assert segments.shape[1] == 4 and tiles.shape[1] == 2 and tile_sumsq.numel() >= tiles.shape[0]
    _check(lib.xv_augment_power_f64(_dev(sig, torch.int16, "sig"), _dev(segments, torch.int64, "segments"),
                                    _dev(tiles, torch.int64, "tiles"), int(tiles.shape[0]), _dev(tile_sumsq, torch.float64, "tile_sumsq"),
                                    _stream()), "xv_augment_power_f64")


def augment_conv(sig, taps, jobs, tiles, y, tile_sumsq):
    """Step 2 (xv_augment_conv_f64): jobs [J, 5], tiles [T, 2] int64; y, tile_sumsq float64 [>= T]."""
    import torch
    lib = require_gpu()
    assert jobs.shape[1] == 5 and tiles.shape[1] == 2 and tile_sumsq.numel() >= tiles.shape[0]
    _check(lib.xv_augment_conv_f64(_dev(sig, torch.int16, "sig"), _dev(taps, torch.float32, "taps"), _dev(jobs, torch.int64, "jobs"),
                                   _dev(tiles, torch.int64, "tiles"), int(tiles.shape[0]), _dev(y, torch.float64, "y"),
                                   _dev(tile_sumsq, torch.float64, "tile_sumsq"), _stream()), "xv_augment_conv_f64")


def augment_gains(utt, refs, ref_snr, segments, power_sumsq, conv_sumsq, utt_out, ref_power, ref_scale):
    """Step 3 (xv_augment_gains_f32): utt [U, 16], refs [R, 4], segments [S, 4] int64 descriptors; utt_out [U, 4] float64."""
    import torch
    lib = require_gpu()
    assert utt.shape[1] == 16 and refs.shape[1] == 4 and segments.shape[1] == 4 and utt_out.shape == (utt.shape[0], 4)
    _check(lib.xv_augment_gains_f32(_dev(utt, torch.int64, "utt"), int(utt.shape[0]), _dev(refs, torch.int64, "refs"),
                                    _dev(ref_snr, torch.float32, "ref_snr"), _dev(segments, torch.int64, "segments"),
                                    _dev(power_sumsq, torch.float64, "power_sumsq"), _dev(conv_sumsq, torch.float64, "conv_sumsq"),
                                    _dev(utt_out, torch.float64, "utt_out"), _dev(ref_power, torch.float64, "ref_power"),
                                    _dev(ref_scale, torch.float32, "ref_scale"), _stream()), "xv_augment_gains_f32")


def augment_mix(sig, utt, refs, ref_scale, tiles, y, tile_sumsq):
    """Step 4 (xv_augment_mix_f64): tiles [T, 2] = (utterance, first sample) int64."""
    import torch
    lib = require_gpu()
    assert tiles.shape[1] == 2 and tile_sumsq.numel() >= tiles.shape[0]
    _check(lib.xv_augment_mix_f64(_dev(sig, torch.int16, "sig"), _dev(utt, torch.int64, "utt"), _dev(refs, torch.int64, "refs"),
                                  _dev(ref_scale, torch.float32, "ref_scale"), _dev(tiles, torch.int64, "tiles"), int(tiles.shape[0]),
                                  _dev(y, torch.float64, "y"), _dev(tile_sumsq, torch.float64, "tile_sumsq"), _stream()),
           "xv_augment_mix_f64")


def augment_level(utt, utt_param, mix_sumsq, utt_out):
    """Step 5 (xv_augment_level_f32): utt_param [U, 2] float64 = (volume, normalize)."""
    import torch
    lib = require_gpu()
    assert utt_param.shape == (utt.shape[0], 2)
    _check(lib.xv_augment_level_f32(_dev(utt, torch.int64, "utt"), int(utt.shape[0]), _dev(utt_param, torch.float64, "utt_param"),
                                    _dev(mix_sumsq, torch.float64, "mix_sumsq"), _dev(utt_out, torch.float64, "utt_out"), _stream()),
           "xv_augment_level_f32")


def augment_write(y, utt, utt_out, tiles, out, sample_format, clipped):
    """Step 6 (xv_augment_write): out int16 (sample_format 0) or float32 (1), 1-D; clipped [U] int64 counters."""
    import torch
    lib = require_gpu()
    assert tiles.shape[1] == 2 and out.dim() == 1 and out.dtype == (torch.int16 if sample_format == 0 else torch.float32)
    _check(lib.xv_augment_write(_dev(y, torch.float64, "y"), _dev(utt, torch.int64, "utt"), _dev(utt_out, torch.float64, "utt_out"),
                                _dev(tiles, torch.int64, "tiles"), int(tiles.shape[0]), _ptr(out), int(sample_format),
                                _dev(clipped, torch.int64, "clipped"), _stream()), "xv_augment_write")


def l2_normalize_rows(x, y=None, norm=None):
    """-> (y = x / ||x|| per row, norms[R]); ``y`` / ``norm`` optional preallocated outputs."""
    import torch
    lib = require_gpu()
    _f32(x, "x")
    y = torch.empty_like(x) if y is None else _f32(y, "y")
    norm = torch.empty(x.shape[0], dtype=torch.float32, device=x.device) if norm is None else _f32(norm, "norm")
    assert y.shape == x.shape and norm.numel() == x.shape[0]
    _check(lib.xv_l2_normalize_rows_f32(_ptr(x), x.stride(0), x.shape[0], x.shape[1], _ptr(y), y.stride(0), _ptr(norm), _stream()),
           "xv_l2_normalize_rows_f32")
    return y, norm


def l2_normalize_backward(dy, y, norm, dx=None):
    import torch
    lib = require_gpu()
    _f32(dy, "dy"); _f32(y, "y"); _f32(norm, "norm")
    assert dy.shape == y.shape and norm.numel() == y.shape[0]
    dx = torch.empty_like(y) if dx is None else _f32(dx, "dx")
    assert dx.shape == y.shape
    _check(lib.xv_l2_normalize_backward_f32(_ptr(dy), _ptr(y), _ptr(norm), y.shape[0], y.shape[1], _ptr(dx), _stream()),
           "xv_l2_normalize_backward_f32")
    return dx


def am_margin(cosines, labels, scale, margin):
    import torch
    lib = require_gpu()
    _f32(cosines, "cosines")
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.numel() == cosines.shape[0]
    _check(lib.xv_am_margin_f32(_ptr(cosines), _ptr(labels), cosines.shape[0], cosines.shape[1], float(scale), float(margin), _stream()),
           "xv_am_margin_f32")


# ------------------------------------------------------------------------------------------------
# self-attentive statistics pooling (local/tf/models.py:1036-1052)
# ------------------------------------------------------------------------------------------------
def attention_scores(u, v, scores, nonlin=None, rows=None):
    """scores[r] = sum_c v[c]*tanh(u[r,c]); nonlin (optional, same shape as u) receives tanh(u)."""
    lib = require_gpu()
    _rows2d(u, "u"); _f32(v, "v"); _f32(scores, "scores")
    R = u.shape[0] if rows is None else int(rows)
    assert v.numel() == u.shape[1] and scores.numel() >= R
    ldn = 0
    if nonlin is not None:
        _rows2d(nonlin, "nonlin"); assert nonlin.shape[1] == u.shape[1] and nonlin.shape[0] >= R
        ldn = nonlin.stride(0)
    _check(lib.xv_attention_scores_f32(_ptr(u), u.stride(0), R, u.shape[1], _ptr(v), _ptr(scores), _ptr(nonlin), ldn, _stream()),
           "xv_attention_scores_f32")


def attention_softmax(scores, row_start, row_len, nchunks, att):
    lib = require_gpu()
    _f32(scores, "scores"); _f32(att, "att")
    _chunk_tables(row_start, row_len)
    assert att.numel() >= scores.numel()
    _check(lib.xv_attention_softmax_f32(_ptr(scores), _ptr(row_start), _ptr(row_len), int(nchunks), _ptr(att), _stream()),
           "xv_attention_softmax_f32")


def attention_pool_workspace_bytes(c, nchunks, max_len, split_rows):
    return int(load().xv_attention_pool_workspace_bytes(int(c), int(nchunks), int(max_len), int(split_rows)))


def attention_pool(h, att, row_start, row_len, nchunks, max_len, split_rows, eps, out, workspace=None):
    """out[b] = [sum_t att h | sqrt(sum_t att h^2 - (sum_t att h)^2 + eps)] over the rows of chunk b; h: [R, C] rows (may be a
    column slice of a wider buffer)."""
    lib = require_gpu()
    _rows2d(h, "h"); _f32(att, "att"); _f32(out, "out")
    _chunk_tables(row_start, row_len)
    c = h.shape[1]
    assert out.shape[1] == 2 * c and out.shape[0] >= nchunks and att.numel() >= h.shape[0]
    need = attention_pool_workspace_bytes(c, nchunks, max_len, split_rows)
    if need:
        assert workspace is not None and _nbytes(workspace) >= need, "attention pool workspace too small"
    _check(lib.xv_attention_pool_f32(_ptr(h), h.stride(0), c, _ptr(att), _ptr(row_start), _ptr(row_len), int(nchunks), int(max_len),
                                     int(split_rows), float(eps), _ptr(out), _ptr(workspace), _stream()), "xv_attention_pool_f32")


def attention_pool_backward(h, att, row_start, row_len, nchunks, max_len, pooled, dpooled, dh, datt):
    """h, dh: [R, C] rows (column slices allowed); pooled, dpooled: [nchunks, 2C]; datt: [R] (only chunk rows are written)."""
    lib = require_gpu()
    _rows2d(h, "h"); _rows2d(dh, "dh"); _f32(att, "att"); _f32(pooled, "pooled"); _f32(dpooled, "dpooled"); _f32(datt, "datt")
    c = h.shape[1]
    assert dh.shape == h.shape and pooled.shape[1] == 2 * c and dpooled.shape == pooled.shape and datt.numel() >= h.shape[0]
    _check(lib.xv_attention_pool_backward_f32(_ptr(h), h.stride(0), c, _ptr(att), _ptr(row_start), _ptr(row_len), int(nchunks),
                                              int(max_len), _ptr(pooled), _ptr(dpooled), _ptr(dh), dh.stride(0), _ptr(datt),
                                              _stream()), "xv_attention_pool_backward_f32")


def attention_softmax_backward(att, datt, row_start, row_len, nchunks, dscores):
    lib = require_gpu()
    _f32(att, "att"); _f32(datt, "datt"); _f32(dscores, "dscores")
    _check(lib.xv_attention_softmax_backward_f32(_ptr(att), _ptr(datt), _ptr(row_start), _ptr(row_len), int(nchunks), _ptr(dscores),
                                                 _stream()), "xv_attention_softmax_backward_f32")


def attention_scores_backward(nonlin, dscores, v, du):
    """du = dscores v (1 - nonlin^2); nonlin <- dscores * nonlin (column sums = dv)."""
    lib = require_gpu()
    _rows2d(nonlin, "nonlin"); _rows2d(du, "du"); _f32(dscores, "dscores"); _f32(v, "v")
    R, c = nonlin.shape
    assert du.shape == nonlin.shape and dscores.numel() >= R and v.numel() == c
    _check(lib.xv_attention_scores_backward_f32(_ptr(nonlin), nonlin.stride(0), _ptr(dscores), _ptr(v), R, c, _ptr(du), du.stride(0),
                                                _stream()), "xv_attention_scores_backward_f32")
