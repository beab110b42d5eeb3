"""ctypes binding of libfil_hip.so (include/fil.h).  No CPU fallback: if the library is missing or a call
fails, the product path raises."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# FIL_LIB_PATH (development only): an alternative build of the SAME library -- kernel experiments built side by side by
# tools/abl_build.py (-> tools/abl/libfil_<name>.so) and timed against the default one in separate processes.  Honoured only for a
# file inside this repository's tools/abl/ directory: the variable cannot point the product at a library from anywhere else.
# Unset (or anything else) = the in-tree default.
def _lib_path():
    default = os.path.join(_HERE, "libfil_hip.so")
    alt = os.environ.get("FIL_LIB_PATH")
    if not alt:
        return default
    abl = os.path.realpath(os.path.join(_HERE, "..", "tools", "abl")) + os.sep
    if os.path.realpath(alt).startswith(abl):
        return alt
    import warnings
    warnings.warn("FIL_LIB_PATH=%s is outside %s: ignored, loading the in-tree libfil_hip.so" % (alt, abl))
    return default


LIB_PATH = _lib_path()
HEADER_PATH = os.path.join(_HERE, "..", "include", "fil.h")

FIL_F32, FIL_BF16 = 0, 1
FIL_ADAM_KERAS, FIL_ADAM_LAZY = 0, 1
FIL_ADAM_ROLL_STEP, FIL_ADAM_ROLL_SKIP, FIL_ADAM_ROLL_FLUSH = 0, 1, 2
FIL_OPT_ADAGRAD, FIL_OPT_FTRL = 1, 2
FIL_OPT_SGD, FIL_OPT_RMSPROP = 3, 4
FIL_MOMOPT_NESTEROV = 1
FIL_OPT_ADADELTA, FIL_OPT_ADAMAX = 5, 6
FIL_OPT_NADAM = 7
FIL_CONFUSION_MAX_T, FIL_CONFUSION_ONE_LAUNCH_N = 2048, 16384
FIL_MEAN_VALUES, FIL_MEAN_BCE, FIL_MEAN_BINARY_ACC = 0, 1, 2
FIL_MEAN_ONE_LAUNCH_N = 16384
FIL_BAG_SUM, FIL_BAG_MEAN, FIL_BAG_SQRTN = 0, 1, 2
FIL_BAG_NO_PAD = -(1 << 63)      # INT64_MIN: no id is padding
FIL_BAG_MAX_BLOCKS = 2048        # fil_embed_bag_fwd's grid cap (workgroups of 256 threads)
FIL_AFM_HIDDEN_RELU = 1          # fil_afm_*'s flag bit 0: s_p = relu(u_p) . h (the paper's form)
FIL_DIN_SOFTMAX, FIL_DIN_SIGMOID = 1, 2   # fil_din_*'s flag bits: softmax over the live slots; sigmoid instead of PReLU
FIL_GRU_GRU, FIL_GRU_AUGRU, FIL_GRU_AGRU = 0, 1, 2   # fil_gru_*'s mode
FIL_LSTM_FORWARD, FIL_LSTM_REVERSE, FIL_LSTM_BIDIR = 0, 1, 2   # fil_lstm_*'s dirs
FIL_SEARCH_PREFER_LAST = 1       # fil_seq_search's flag bit 0: among equal scores the later positions win
FIL_SEQ_VIEW_FULL, FIL_SEQ_VIEW_CAUSAL, FIL_SEQ_VIEW_CROSS = 0, 1, 2      # fil_seqattn_*_v's structure masks
FIL_ERR_UNSUPPORTED = -4

_c = ctypes
_P = _c.c_void_p
_I = _c.c_int
_Z = _c.c_size_t
_F = _c.c_float
_L = _c.c_int64

# name -> (restype, argtypes); mirrors include/fil.h one to one
SIGNATURES = {
    "fil_version": (_I, []),
    "fil_last_error": (_c.c_char_p, []),
    "fil_profile_begin": (_I, [_c.c_char_p]),
    "fil_profile_end": (_Z, [_c.c_char_p, _Z]),
    "fil_fm_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "fil_fm_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "fil_fm_pairs_fwd": (_I, [_P, _P, _I, _I, _I, _P]),
    "fil_fm_pairs_bwd": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "fil_dcn_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "fil_dcn_bwd_workspace_bytes": (_Z, [_I, _I, _I]),
    "fil_dcn_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "fil_cin_saved_bytes": (_Z, [_I, _I, _I, _I, _P]),
    "fil_cin_fwd_workspace_bytes": (_Z, [_I, _I, _I, _I, _P]),
    "fil_cin_bwd_workspace_bytes": (_Z, [_I, _I, _I, _I, _P]),
    "fil_cin_grad_ready_points": (_I, [_I, _I, _I, _I, _P, _I, _P]),
    "fil_cin_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P, _Z, _P]),
    "fil_cin_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P, _P, _Z, _P]),
    "fil_cin_precision_used": (_I, [_I, _I, _I, _I, _P, _I, _I]),
    "fil_cin_shortdx_used": (_I, [_I, _I, _I, _I, _P, _I, _I, _I]),
    "fil_cin_fwd_p": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _Z, _P]),
    "fil_cin_bwd_p": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _Z, _P]),
    "fil_attn_plan": (_I, [_I, _I, _I, _I, _I, _P]),
    "fil_attn_fwd_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "fil_attn_bwd_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I]),
    "fil_attn_fwd": (_I, [_P] * 10 + [_I, _I, _I, _I, _I, _F, _F, _I, _I, _I, _P, _Z, _P]),
    "fil_attn_bwd": (_I, [_P] * 17 + [_I, _I, _I, _I, _I, _F, _F, _I, _I, _I, _P, _Z, _P]),
    "fil_pattn_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P]),
    "fil_pattn_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P]),
    "fil_embed_gather": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "fil_embed_gather_dt": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "fil_embed_gather_xt": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "fil_embed_scatter_add": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "fil_embed_row_ids": (_I, [_P, _P, _P, _P, _P, _I, _I, _P]),
    "fil_embed_sort_fields": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _c.c_int64, _P]),
    "fil_embed_segment_sum": (_I, [_P, _P, _P, _P, _P, _P, _c.c_long, _I, _P]),
    "fil_embed_run_sum": (_I, [_P, _P, _P, _P, _c.c_long, _I, _P]),
    "fil_embed_run_sum_dt": (_I, [_P, _P, _P, _P, _c.c_long, _I, _I, _P]),
    # N3: pooled multi-valued fields
    "fil_embed_bag_fwd": (_I, [_P, _P, _P, _P, _c.c_int64, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "fil_embed_bag_row_ids": (_I, [_P, _P, _P, _P, _c.c_int64, _P, _I, _I, _I, _P]),
    "fil_embed_bag_bwd_prep": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    # N3: AFM pair-attention pooling (softmax over the pairs)
    "fil_afm_plan": (_I, [_I, _I, _I, _I, _P]),
    "fil_afm_fwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "fil_afm_bwd_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "fil_afm_bwd": (_I, [_P] * 12 + [_Z, _I, _I, _I, _I, _I, _P]),
    # N3: DIN attention pooling over a behaviour sequence
    "fil_din_plan": (_I, [_I, _I, _I, _I, _I, _P]),
    "fil_din_fwd": (_I, [_P] * 13 + [_I] * 6 + [_P]),
    "fil_din_bwd_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "fil_din_bwd": (_I, [_P] * 25 + [_Z] + [_I] * 6 + [_P]),
    # N3: GRU / AUGRU / AGRU over a behaviour sequence
    "fil_gru_plan": (_I, [_I, _I, _I, _I, _I, _P]),
    "fil_gru_saved_bytes": (_Z, [_I, _I, _I, _I]),
    "fil_gru_fwd": (_I, [_P] * 8 + [_I] * 5 + [_P]),
    "fil_gru_bwd_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "fil_gru_bwd": (_I, [_P] * 15 + [_Z] + [_I] * 5 + [_P]),
    # N3: LSTM over a sequence, one direction or both in one launch
    "fil_lstm_plan": (_I, [_I, _I, _I, _I, _I, _P]),
    "fil_lstm_saved_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "fil_lstm_fwd": (_I, [_P] * 7 + [_I] * 5 + [_P]),
    "fil_lstm_bwd_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "fil_lstm_bwd": (_I, [_P] * 13 + [_Z] + [_I] * 5 + [_P]),
    # N3: masked multi-head self-attention over a behaviour sequence
    "fil_seqattn_plan": (_I, [_I, _I, _I, _I, _I, _P]),
    "fil_seqattn_saved_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "fil_seqattn_fwd": (_I, [_P] * 7 + [_I] * 6 + [_P]),
    "fil_seqattn_bwd_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "fil_seqattn_bwd": (_I, [_P] * 13 + [_Z] + [_I] * 6 + [_P]),
    "fil_seqattn_fwd_v": (_I, [_P] * 8 + [_I] * 8 + [_P]),
    "fil_seqattn_bwd_v": (_I, [_P] * 13 + [_Z] + [_I] * 8 + [_P]),
    # N3: top-k retrieval over a long behaviour history (forward only)
    "fil_seq_search_plan": (_I, [_I, _I, _I, _I, _P]),
    "fil_seq_search": (_I, [_P, _L, _L, _L, _L, _P, _P, _P, _L, _P, _L, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    # N4: Neural Turing Machine memory read / write over a sequence
    "fil_ntm_plan": (_I, [_I, _I, _I, _I, _I, _P]),
    "fil_ntm_saved_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "fil_ntm_fwd": (_I, [_P] * 9 + [_I] * 5 + [_P]),
    "fil_ntm_bwd_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "fil_ntm_bwd": (_I, [_P] * 12 + [_Z] + [_I] * 5 + [_P]),
    # N5: time-stream GRU over a behaviour sequence with event gaps
    "fil_tsgru_plan": (_I, [_I, _I, _I, _I, _I, _P]),
    "fil_tsgru_saved_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "fil_tsgru_fwd": (_I, [_P] * 12 + [_I] * 5 + [_P]),
    "fil_tsgru_bwd_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "fil_tsgru_bwd": (_I, [_P] * 18 + [_Z] + [_I] * 5 + [_P]),
    "fil_score_add_sigmoid_fwd": (_I, [_P, _P, _P, _P, _P, _I, _P]),
    "fil_score_add_sigmoid_bwd": (_I, [_P, _P, _P, _I, _P]),
    "fil_bce_mean_fwd": (_I, [_P, _P, _F, _P, _P, _I, _P]),
    "fil_gemm_f32_workspace_bytes": (_Z, [_I, _I, _I]),
    "fil_gemm_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "fil_relu_bias_bwd_workspace_bytes": (_Z, [_I, _I]),
    "fil_relu_bias_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "fil_merge_softmax_bwd_workspace_bytes": (_Z, [_I, _I, _I]),
    "fil_merge_softmax_fwd": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _I, _P]),
    "fil_merge_softmax_bwd": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P]),
    "fil_adam_multi": (_I, [_P, _I, _c.c_int64, _P, _F, _F, _F, _F, _I, _P]),
    "fil_embed_adam_runs": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _F, _F, _F, _F, _I, _P]),
    "fil_embed_adam_sweep": (_I, [_P, _P, _P, _P, _c.c_int64, _I, _P, _P, _P, _I, _P, _F, _F, _F, _F, _P]),
    "fil_embed_runs_compact_workspace_bytes": (_Z, [_c.c_long]),
    "fil_embed_runs_compact": (_I, [_P, _P, _P, _c.c_long, _I, _I, _P, _P, _P, _c.c_long, _P, _Z, _P]),
    "fil_embed_adam_merged": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _I, _P, _P, _P, _P, _c.c_int64, _P, _F, _F, _F, _F, _I, _P]),
    "fil_embed_adam_ring_len": (_I, [_I]),
    "fil_embed_adam_catchup_runs": (_I, [_P, _c.c_long, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _c.c_int64, _P, _P]),
    "fil_embed_adam_runs_deferred": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _c.c_int64, _P, _F, _F,
                                          _F, _F, _P]),
    "fil_embed_adam_merged_deferred": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _c.c_int64, _P, _F,
                                            _F, _F, _F, _P]),
    "fil_embed_adam_roll": (_I, [_P, _P, _P, _P, _P, _I, _c.c_int64, _I, _P, _P, _P, _I, _P, _F, _F, _F, _F, _I, _P]),
    "fil_rowopt_multi": (_I, [_P, _I, _c.c_int64, _P, _I, _P, _I, _P]),
    "fil_embed_rowopt_runs": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "fil_embed_rowopt_sweep": (_I, [_P, _P, _P, _P, _c.c_int64, _I, _P, _P, _P, _I, _P, _I, _P, _P]),
    "fil_embed_rowopt_merged": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _I, _P, _P, _P, _P, _c.c_int64, _P, _I, _P, _P]),
    # O3: the evaluation of a schedule and the device-rate variants (lr_dev in place of lr; beside the hyper for the rowwise rules)
    "fil_lr_schedule_check": (_I, [_P]),
    "fil_lr_schedule_eval": (_I, [_P, _P, _P, _P]),
    "fil_adam_multi_lrdev": (_I, [_P, _I, _c.c_int64, _P, _P, _F, _F, _F, _I, _P]),
    "fil_embed_adam_runs_lrdev": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _F, _F, _I, _P]),
    "fil_embed_adam_sweep_lrdev": (_I, [_P, _P, _P, _P, _c.c_int64, _I, _P, _P, _P, _I, _P, _P, _F, _F, _F, _P]),
    "fil_embed_adam_merged_lrdev": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _I, _P, _P, _P, _P, _c.c_int64, _P, _P, _F, _F, _F, _I, _P]),
    "fil_embed_adam_runs_deferred_lrdev": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _c.c_int64, _P, _P,
                                                _F, _F, _F, _P]),
    "fil_embed_adam_merged_deferred_lrdev": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _c.c_int64, _P, _P,
                                                  _F, _F, _F, _P]),
    "fil_embed_adam_roll_lrdev": (_I, [_P, _P, _P, _P, _P, _I, _c.c_int64, _I, _P, _P, _P, _I, _P, _P, _F, _F, _F, _I, _P]),
    "fil_rowopt_multi_lrdev": (_I, [_P, _I, _c.c_int64, _P, _I, _P, _P, _I, _P]),
    "fil_embed_rowopt_runs_lrdev": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "fil_embed_rowopt_sweep_lrdev": (_I, [_P, _P, _P, _P, _c.c_int64, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P]),
    "fil_embed_rowopt_merged_lrdev": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _I, _P, _P, _P, _P, _c.c_int64, _P, _I, _P, _P, _P]),
    # O4: SGD / RMSprop -- the argument lists of the O2 entry points, with a fil_momopt_hyper
    "fil_momopt_multi": (_I, [_P, _I, _c.c_int64, _P, _I, _P, _I, _P]),
    "fil_embed_momopt_runs": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "fil_embed_momopt_sweep": (_I, [_P, _P, _P, _P, _c.c_int64, _I, _P, _P, _P, _I, _P, _I, _P, _P]),
    "fil_embed_momopt_merged": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _I, _P, _P, _P, _P, _c.c_int64, _P, _I, _P, _P]),
    "fil_momopt_multi_lrdev": (_I, [_P, _I, _c.c_int64, _P, _I, _P, _P, _I, _P]),
    "fil_embed_momopt_runs_lrdev": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "fil_embed_momopt_sweep_lrdev": (_I, [_P, _P, _P, _P, _c.c_int64, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P]),
    "fil_embed_momopt_merged_lrdev": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _I, _P, _P, _P, _P, _c.c_int64, _P, _I, _P, _P, _P]),
    # O5: Adadelta / Adamax -- the argument lists of the O4 entry points, with a fil_adaopt_hyper
    "fil_adaopt_multi": (_I, [_P, _I, _c.c_int64, _P, _I, _P, _I, _P]),
    "fil_embed_adaopt_runs": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "fil_embed_adaopt_sweep": (_I, [_P, _P, _P, _P, _c.c_int64, _I, _P, _P, _P, _I, _P, _I, _P, _P]),
    "fil_embed_adaopt_merged": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _I, _P, _P, _P, _P, _c.c_int64, _P, _I, _P, _P]),
    "fil_adaopt_multi_lrdev": (_I, [_P, _I, _c.c_int64, _P, _I, _P, _P, _I, _P]),
    "fil_embed_adaopt_runs_lrdev": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "fil_embed_adaopt_sweep_lrdev": (_I, [_P, _P, _P, _P, _c.c_int64, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P]),
    "fil_embed_adaopt_merged_lrdev": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _I, _P, _P, _P, _P, _c.c_int64, _P, _I, _P, _P, _P]),
    # O6: Nadam -- the argument lists of the O4 entry points, with a fil_nadam_hyper; no _lrdev twins
    "fil_nadam_multi": (_I, [_P, _I, _c.c_int64, _P, _I, _P, _I, _P]),
    "fil_embed_nadam_runs": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "fil_embed_nadam_sweep": (_I, [_P, _P, _P, _P, _c.c_int64, _I, _P, _P, _P, _I, _P, _I, _P, _P]),
    "fil_embed_nadam_merged": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _I, _P, _P, _P, _P, _c.c_int64, _P, _I, _P, _P]),
    # O7: Adam with amsgrad -- O1's Keras-mode argument lists with vhat behind v and (lr, lr_dev) in place of lr; no _lrdev twins
    "fil_amsgrad_multi": (_I, [_P, _I, _c.c_int64, _P, _F, _P, _F, _F, _F, _I, _P]),
    "fil_embed_amsgrad_runs": (_I, [_P, _P, _P, _c.c_long, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _P, _F, _F, _F, _P]),
    "fil_embed_amsgrad_sweep": (_I, [_P, _P, _P, _P, _P, _c.c_int64, _I, _P, _P, _P, _I, _P, _F, _P, _F, _F, _F, _P]),
    "fil_embed_amsgrad_merged": (_I, [_P, _P, _P, _I, _c.c_long, _I, _P, _P, _I, _P, _P, _P, _P, _P, _c.c_int64, _P, _F, _P, _F, _F, _F,
                                      _P]),
    "fil_confusion_workspace_bytes": (_Z, [_I, _I]),
    "fil_confusion_update": (_I, [_P, _P, _I, _P, _I, _P, _P, _P, _Z, _P]),
    "fil_auc_result": (_I, [_P, _I, _I, _I, _P, _P]),
    "fil_mean_workspace_bytes": (_Z, [_I]),
    "fil_mean_update": (_I, [_I, _P, _P, _I, _F, _F, _P, _P, _Z, _P]),
}


class RowoptHyper(_c.Structure):
    """fil_rowopt_hyper (include/fil.h O2)"""
    _fields_ = [("lr", _F), ("epsilon", _F), ("lr_power", _F), ("l1", _F), ("l2", _F), ("l2_shrinkage", _F)]


class MomoptHyper(_c.Structure):
    """fil_momopt_hyper (include/fil.h O4)"""
    _fields_ = [("lr", _F), ("epsilon", _F), ("rho", _F), ("momentum", _F), ("flags", _c.c_int32), ("reserved", _c.c_int32)]


assert _c.sizeof(MomoptHyper) == 24


class AdaoptHyper(_c.Structure):
    """fil_adaopt_hyper (include/fil.h O5)"""
    _fields_ = [("lr", _F), ("rho", _F), ("beta_1", _F), ("beta_2", _F), ("epsilon", _F)]


assert _c.sizeof(AdaoptHyper) == 20


class NadamHyper(_c.Structure):
    """fil_nadam_hyper (include/fil.h O6); m_cache: the device address of the momentum cache word"""
    _fields_ = [("lr", _F), ("beta_1", _F), ("beta_2", _F), ("epsilon", _F), ("schedule_decay", _F), ("reserved", _c.c_int32),
                ("m_cache", _P)]


assert _c.sizeof(NadamHyper) == 32


class AmsgradTensor(_c.Structure):
    """fil_amsgrad_tensor (include/fil.h O7)"""
    _fields_ = [("param", _P), ("grad", _P), ("m", _P), ("v", _P), ("vhat", _P), ("numel", _c.c_int64), ("l2", _F),
                ("reserved", _c.c_int32)]


assert _c.sizeof(AmsgradTensor) == 56

FIL_LR_CONSTANT, FIL_LR_EXPONENTIAL, FIL_LR_INVERSE_TIME, FIL_LR_POLYNOMIAL, FIL_LR_PIECEWISE = 0, 1, 2, 3, 4
FIL_LR_MAX_BOUNDARIES = 32


class LrSchedule(_c.Structure):
    """fil_lr_schedule (include/fil.h O3)"""
    _fields_ = [("kind", _c.c_int32), ("flag", _c.c_int32), ("initial_lr", _F), ("decay_steps", _F), ("decay_rate", _F), ("end_lr", _F),
                ("power", _F), ("decay", _F), ("n_boundaries", _c.c_int32), ("reserved", _c.c_int32),
                ("boundaries", _c.c_int64 * FIL_LR_MAX_BOUNDARIES), ("values", _F * (FIL_LR_MAX_BOUNDARIES + 1)), ("reserved2", _c.c_int32)]


assert _c.sizeof(LrSchedule) == 432


class FilError(RuntimeError):
    pass


_lib = None


def header_symbols():
    """Names of every function declared in include/fil.h."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fil_[a-z0-9_]+)\s*\(", text)))


def header_abi_version():
    """FIL_ABI_VERSION of include/fil.h (the version this binding's SIGNATURES table was written against)."""
    m = re.search(r"#define\s+FIL_ABI_VERSION\s+(\d+)", open(HEADER_PATH).read())
    if m is None:
        raise FilError("include/fil.h does not define FIL_ABI_VERSION")
    return int(m.group(1))


def load():
    """Loads libfil_hip.so (raises FilError if it has not been built: python -m ml_function_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FilError("libfil_hip.so not found at %s -- build it with `python -m ml_function_amd.build` "
                       "(there is no CPU fallback)" % LIB_PATH)
    # torch first: it ships its own libamdhip64, and the process must end up with ONE HIP runtime -- loaded the other way round
    # (this library pulling in /opt/rocm's copy before torch brings its own) every launch fails with "no ROCm-capable device"
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    missing = [name for name in SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise FilError("libfil_hip.so at %s does not export %s -- rebuild it (python -m ml_function_amd.build --force)"
                       % (LIB_PATH, ", ".join(missing)))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    want = header_abi_version()
    if lib.fil_version() != want:
        raise FilError("libfil_hip.so at %s has ABI version %d, include/fil.h says %d -- stale build, rebuild it "
                       "(python -m ml_function_amd.build --force)" % (LIB_PATH, lib.fil_version(), want))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().fil_last_error().decode("utf-8", "replace")
        raise FilError("%s failed (%d): %s" % (what, rc, msg))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    """hipStream_t of torch's current stream on the current device, as an integer (the raw getter: no Stream object is built --
    this runs once per C-ABI call)."""
    import torch
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def int_array(vals):
    return (ctypes.c_int * len(vals))(*vals)


def ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def profile_begin(filter=None):
    """Start per-kernel event timing; filter = "substr,substr" restricts it to the scopes whose name contains one."""
    load().fil_profile_begin(None if not filter else filter.encode())


def profile_end():
    """Returns {kernel name: dict(count, total_ms, avg_ms, work, executed)} for the launches since profile_begin():
    work = algorithmic flops / bytes per launch (the reference graph's), executed = what the kernels of the scope compute."""
    lib = load()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.fil_profile_end(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, count, ms, work, executed = line.split()
        out[name] = dict(count=int(count), total_ms=float(ms), avg_ms=float(ms) / max(int(count), 1), work=float(work),
                         executed=float(executed))
    return out
