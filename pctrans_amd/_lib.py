"""ctypes binding of libpctrans_hip.so (C ABI: include/pctrans_hip.h).  Fails loudly if the library is missing."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpctrans_hip.so")
ABI_VERSION = 1

_lib = None

_vp, _i = ctypes.c_void_p, ctypes.c_int
_FWD_ARGS = [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]
_BWD_ARGS = [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]

SYMBOLS = {
    "pct_abi_version": ([], _i),
    "pct_error_string": ([_i], ctypes.c_char_p),
    "pct_build_info": ([], ctypes.c_char_p),
    "pct_prepare_device": ([], _i),
    "pct_ms_deform_attn_forward_f32": (_FWD_ARGS, _i),
    "pct_ms_deform_attn_forward_f64": (_FWD_ARGS, _i),
    "pct_ms_deform_attn_forward_f16": (_FWD_ARGS, _i),
    "pct_ms_deform_attn_forward_bf16": (_FWD_ARGS, _i),
    "pct_ms_deform_attn_backward_f32": (_BWD_ARGS, _i),
    "pct_ms_deform_attn_backward_f64": (_BWD_ARGS, _i),
    "pct_ms_deform_attn_fused_forward_f32": ([_vp, _vp, _vp, _vp, ctypes.c_longlong, _vp, _vp] + [_i] * 7 + [_vp, _vp], _i),
    "pct_ms_deform_attn_forward_planes_f32": ([_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_longlong] + [_i] * 7 + [_vp, _vp], _i),
    "pct_add_layernorm_f32": ([_vp, _vp, _vp, _vp, ctypes.c_float, ctypes.c_longlong, _i, _vp, _vp], _i),
    "pct_linear_k128_f32": ([_vp, ctypes.c_longlong, _vp, ctypes.c_longlong, ctypes.c_longlong, _vp, _vp, ctypes.c_longlong, _i, _i, _vp,
                             ctypes.c_longlong, _vp], _i),
    "pct_msda_set_kernel_choice": ([_i], None),
    "pct_msda_last_kernel": ([], _i),
    "pct_msda_set_bwd_kernel_choice": ([_i], None),
    "pct_msda_last_bwd_kernel": ([], _i),
    "pct_linear_k128_multi_f32": ([_vp, ctypes.c_longlong, _vp, ctypes.c_longlong, ctypes.c_longlong, _i, _vp, _vp, _vp, _vp,
                                   _vp, _vp, ctypes.c_longlong, _vp], _i),
    "pct_linear_k128_add_layernorm_f32": ([_vp, ctypes.c_longlong, _vp, _vp, _vp, ctypes.c_longlong, _vp, _vp,
                                           ctypes.c_float, ctypes.c_longlong, _vp, ctypes.c_longlong, _vp], _i),
    "pct_linear_add_layernorm_f32": ([_vp, ctypes.c_longlong, _i, _vp, _vp, _vp, _vp, ctypes.c_longlong, _vp, _vp,
                                      ctypes.c_float, ctypes.c_longlong, _vp, ctypes.c_longlong, _vp], _i),
    "pct_groupnorm_flatten_f32": ([_vp, _vp, _vp, _i, _i, _i, _i, ctypes.c_float, _vp, _vp, ctypes.c_longlong,
                                   ctypes.c_longlong, _vp], _i),
    "pct_conv1x1_nchw_f32": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp], _i),
    "pct_conv1x1_groupnorm_tokens_f32": ([_vp] * 6 + [_i, ctypes.c_float] + [_i] * 4 + [_vp, _vp, _vp, ctypes.c_longlong,
                                          ctypes.c_longlong, _vp], _i),
    "pct_ffn_layernorm_f32": ([_vp, ctypes.c_longlong, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_float, _i, ctypes.c_longlong, _vp, _vp,
                               ctypes.c_longlong, _vp], _i),
    "pct_lsap_f32": ([_vp, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "pct_cross_attention_bf16": ([_vp] * 7 + [_i] * 4 + [ctypes.c_float, _vp, _vp], _i),
    "pct_masked_attention_bf16": ([_vp, _vp, _vp, _vp] + [_i] * 6 + [ctypes.c_float, _i, _vp, _vp], _i),
    "pct_dynamic_mask_head_forward_mfma": ([_vp, _vp, _vp] + [_i] * 9 + [_vp, _vp, _vp, _vp], _i),
    "pct_dynamic_mask_head_forward_fused_bf16": ([_vp, _vp, _vp] + [_i] * 9 + [_vp, _vp, _vp, _vp], _i),
    "pct_dynamic_mask_head_forward": ([_vp, _vp, _vp] + [_i] * 10 + [_vp, _vp, _vp], _i),
}

# Entry points of opt-in paths: no default call site of the head or of a training step reaches them, so they are bound here and
# not in SYMBOLS (whose compute entries are each checked at a default call site).  name -> (argtypes, restype, the test module
# that checks the entry against float64)
OPT_IN_SYMBOLS = {
    "pct_dynamic_mask_head_backward_f32": ([_vp, _vp, _vp, _vp] + [_i] * 7 + [_vp, _vp, _vp, _vp, _vp], _i,
                                           "tests/test_dmh_train_gpu.py"),
    "pct_point_sample_f32": ([_vp, _vp, _vp] + [_i] * 7 + [_vp, _vp], _i, "tests/test_point_loss_gpu.py"),
    "pct_point_mask_loss_forward_f32": ([_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp], _i,
                                        "tests/test_point_loss_gpu.py"),
    "pct_point_mask_loss_backward_f32": ([_vp] * 6 + [_i] * 4 + [_vp, _vp], _i, "tests/test_point_loss_gpu.py"),
    "pct_point_select_uncertain_f32": ([_vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _vp, _i, _vp, _vp], _i,
                                       "tests/test_point_select_gpu.py"),
    "pct_point_match_cost_f32": ([_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _i, ctypes.c_float, ctypes.c_float,
                                  _vp, _vp, _vp], _i, "tests/test_match_cost_gpu.py"),
    # several prediction heads in one launch: the first argument is a host array of device pointers (`head_table`)
    "pct_point_select_uncertain_many_f32": ([_vp, _i, _vp, _i, _i, _i, _vp, _i, _i, _i, _vp, _i, _vp, _vp], _i,
                                            "tests/test_loss_heads_gpu.py"),
    "pct_point_mask_loss_forward_many_f32": ([_vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp], _i,
                                             "tests/test_loss_heads_gpu.py"),
    "pct_point_match_cost_many_f32": ([_vp, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _i, ctypes.c_float,
                                       ctypes.c_float, _vp, _vp, _vp], _i, "tests/test_loss_heads_gpu.py"),
    "pct_instance_label_map_f32": ([_vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp], _i, "tests/test_embedding_loss_gpu.py"),
    "pct_discriminative_loss_forward_f32": ([_vp, _vp] + [_i] * 5 + [ctypes.c_float] * 5 + [_vp] * 5, _i,
                                            "tests/test_embedding_loss_gpu.py"),
    "pct_discriminative_loss_backward_f32": ([_vp] * 4 + [_i] * 5 + [ctypes.c_float, _vp, _vp], _i,
                                             "tests/test_embedding_loss_gpu.py"),
}

# Entry points of the opt-in instance post-processing (include/pctrans_hip_post.h; pctrans_amd/postprocess.py, reached with
# MaskFormer.postprocess = "hip").  A table of its own: SYMBOLS entries each have a default call site, OPT_IN_SYMBOLS is the
# training header's.  name -> (argtypes, restype, the test module that checks the entry)
_POST_MASKS = [_vp] + [_i] * 7 + [_vp, _vp, _vp]
_POST_LABELS = [_vp] + [_i] * 7 + [_vp, _vp, _vp]
POST_SYMBOLS = {
    "pct_instance_masks_f32": (_POST_MASKS, _i, "tests/test_postprocess_gpu.py"),
    "pct_instance_masks_bf16": (_POST_MASKS, _i, "tests/test_postprocess_gpu.py"),
    "pct_instance_labels_from_bits": ([_vp, _vp] + [_i] * 5 + [_vp, _vp, _vp], _i, "tests/test_postprocess_gpu.py"),
    "pct_instance_labels_f32": (_POST_LABELS, _i, "tests/test_postprocess_gpu.py"),
    "pct_instance_labels_bf16": (_POST_LABELS, _i, "tests/test_postprocess_gpu.py"),
}

# Entry points of the semantic head in eval mode (include/pctrans_hip_seg.h; fused_ops.seg_head_forward, the decoder's default
# on bf16 maps with gradients disabled).  A table of its own, as the post-processing's: name -> (argtypes, restype, the test
# module that checks the entry against float64)
SEG_SYMBOLS = {
    "pct_conv3x3_bn_relu_bf16": ([_vp] * 6 + [ctypes.c_float, _vp] + [_i] * 5 + [_vp, _vp], _i, "tests/test_seg_head_gpu.py"),
    "pct_seg_head_bf16": ([_vp] * 6 + [ctypes.c_float] + [_vp] * 5 + [ctypes.c_float] + [_vp] * 4 + [_i] * 5 + [_vp, _vp], _i,
                          "tests/test_seg_head_gpu.py"),
}

# Entry point of the pixel decoder's FPN level in eval mode (include/pctrans_hip_fpn.h; fused_ops.fpn_stage, reached with
# MSDeformAttnPixelDecoder.fpn = "hip").  A table of its own, as the semantic head's: name -> (argtypes, restype, the test module
# that checks the entry against float64)
_FPN_CONV = [_vp] * 6 + [ctypes.c_float]                          # w, bias, mean, var, gamma, beta, eps
FPN_SYMBOLS = {
    "pct_fpn_stage_f32": ([_vp, _vp, ctypes.c_longlong, _i] + _FPN_CONV + _FPN_CONV + [_vp, _vp] + [_i] * 5 + [_vp, _vp], _i,
                          "tests/test_fpn_stage_gpu.py"),
}

# Entry points of the differentiable fp32 cross-attention (include/pctrans_hip_attn_train.h; pctrans_amd/attention_train.py, reached
# with CrossAttentionLayer.attn_train = "hip").  A table of its own, as the FPN level's: name -> (argtypes, restype, the test
# module that checks the entry against float64)
ATTN_TRAIN_SYMBOLS = {
    "pct_cross_attention_forward_f32": ([_vp] * 7 + [_i] * 4 + [ctypes.c_float, _vp, _vp, _vp], _i,
                                        "tests/test_attention_train_gpu.py"),
    "pct_cross_attention_backward_f32": ([_vp] * 10 + [_i] * 4 + [ctypes.c_float] + [_vp] * 7, _i,
                                         "tests/test_attention_train_gpu.py"),
}

# Entry points of the same cross-attention with the keys of every query-side workgroup divided over several workgroups
# (include/pctrans_hip_attn_train_split.h; pctrans_amd/split_key_attention_train.py, reached with
# CrossAttentionLayer.attn_train_split = "hip").  A table of its own, as the unsplit entries': name -> (argtypes, restype, the test
# module that checks the entry against those entries, bit for bit, and against float64)
ATTN_TRAIN_SPLIT_SYMBOLS = {
    "pct_cross_attention_split_train_workspace": ([_i] * 4, ctypes.c_longlong, "tests/test_split_key_attention_train_gpu.py"),
    "pct_cross_attention_split_forward_f32": ([_vp] * 7 + [_i] * 4 + [ctypes.c_float, _i, _vp, ctypes.c_longlong, _vp, _vp, _vp], _i,
                                              "tests/test_split_key_attention_train_gpu.py"),
    "pct_cross_attention_split_backward_f32": ([_vp] * 10 + [_i] * 4 + [ctypes.c_float, _i, _vp, ctypes.c_longlong] + [_vp] * 6, _i,
                                               "tests/test_split_key_attention_train_gpu.py"),
}

# Entry points of the mask side of the query-contrast loss (include/pctrans_hip_reid.h; pctrans_amd/reid_dice.py, reached with
# MultiScaleMaskedTransformerDecoder.reid_dice = "hip").  A table of its own, as the attention's: name -> (argtypes, restype,
# the test module that checks the entry against float64)
REID_SYMBOLS = {
    "pct_reid_dice_rows_forward_f32": ([_vp] * 3 + [_i] * 5 + [_vp] * 5, _i, "tests/test_reid_dice_gpu.py"),
    "pct_reid_dice_rows_backward_f32": ([_vp] * 6 + [_i] * 5 + [_vp] * 3, _i, "tests/test_reid_dice_gpu.py"),
}

# Entry points of the query side of the query-contrast loss and of the per-item reduction of both sides
# (include/pctrans_hip_reid_query.h; pctrans_amd/reid_query.py, reached with MultiScaleMaskedTransformerDecoder.reid_query = "hip"
# and SetCriterion.contrast_loss = "hip").  A table of its own, as the mask side's: name -> (argtypes, restype, the test module
# that checks the entry against float64)
REID_QUERY_SYMBOLS = {
    "pct_reid_nearest_positive_f32": ([_vp, _vp] + [_i] * 4 + [_vp, _vp], _i, "tests/test_reid_query_gpu.py"),
    "pct_reid_query_rows_forward_f32": ([_vp] * 3 + [_i] * 4 + [_vp] * 4, _i, "tests/test_reid_query_gpu.py"),
    "pct_reid_query_rows_backward_f32": ([_vp] * 7 + [_i] * 4 + [_vp] * 3, _i, "tests/test_reid_query_gpu.py"),
    "pct_contrast_loss_rows_f32": ([_vp] * 4 + [_i] * 3 + [ctypes.c_float] + [_vp] * 3, _i, "tests/test_reid_query_gpu.py"),
}

# Entry points of the instance targets from label maps (include/pctrans_hip_targets.h; pctrans_amd/targets.py:
# prepare_instance_targets, MaskFormer.prepare_instance_targets).  A table of its own, as the re-id loss's: name -> (argtypes,
# restype, the test module that checks the entry -- against the torch formulation: the outputs are exact)
TARGETS_SYMBOLS = {
    "pct_instance_targets_census": ([_vp] + [_i] * 5 + [_vp] * 7, _i, "tests/test_targets_gpu.py"),
    "pct_instance_targets_planes": ([_vp] + [_i] * 4 + [_vp, _vp, ctypes.c_longlong, _i] + [_vp] * 5, _i,
                                    "tests/test_targets_gpu.py"),
}

# Entry point of the backward of the fused MSDeformAttn front-end (include/pctrans_hip_msda_train.h; pctrans_amd/msda_train.py,
# reached with MSDeformAttn.train_front = "hip").  A table of its own, as the targets': name -> (argtypes, restype, the test
# module that checks the entry against float64)
MSDA_TRAIN_SYMBOLS = {
    "pct_ms_deform_attn_fused_backward_f32": ([_vp] * 4 + [ctypes.c_longlong] + [_vp] * 3 + [_i] * 8 + [_vp] * 5, _i,
                                              "tests/test_msda_fused_train_gpu.py"),
}

# Entry points of the validation metrics from label maps (include/pctrans_hip_metrics.h; pctrans_amd/metrics.py,
# MaskFormer.validation_metrics).  A table of its own, as the targets': name -> (argtypes, restype, the test module that checks
# the entry -- against the literal per-mask definitions: the integer outputs are exact)
METRICS_SYMBOLS = {
    "pct_label_overlap": ([_vp, _i, _vp, _i, _vp] + [_i] * 3 + [_vp] * 8, _i, "tests/test_metrics_gpu.py"),
    "pct_label_metrics": ([_vp] * 5 + [_i] + [_vp] * 3, _i, "tests/test_metrics_gpu.py"),
}

# Entry points of the differentiable fp32 self-attention (include/pctrans_hip_self_attn_train.h; pctrans_amd/self_attention_train.py,
# reached with SelfAttentionLayer.self_attn_train = "hip").  A table of its own, as the cross-attention's: name -> (argtypes,
# restype, the test module that checks the entry against float64)
SELF_ATTN_TRAIN_SYMBOLS = {
    "pct_self_attention_forward_f32": ([_vp] * 5 + [_i] * 3 + [ctypes.c_float, _vp, _vp, _vp], _i,
                                       "tests/test_self_attention_train_gpu.py"),
    "pct_self_attention_backward_f32": ([_vp] * 8 + [_i] * 3 + [ctypes.c_float] + [_vp] * 5, _i,
                                        "tests/test_self_attention_train_gpu.py"),
}

# Entry points of the criterion's reference-point and semantic losses (include/pctrans_hip_aux_loss.h; pctrans_amd/aux_loss.py:
# refpoint_l1_losses, sem_focal_loss; SetCriterion does not call them yet).  A table of its own, as the self-attention's:
# name -> (argtypes, restype, the test module that checks the entry against float64)
AUX_LOSS_SYMBOLS = {
    "pct_refpoint_l1_forward_f32": ([_vp] * 4 + [_i, ctypes.c_longlong, _i, _i, _i, ctypes.c_float, _vp, _vp, _vp], _i,
                                    "tests/test_aux_loss_gpu.py"),
    "pct_refpoint_l1_backward_f32": ([_vp] * 5 + [_i, ctypes.c_longlong, _i, _i, _i, ctypes.c_float, _vp, _vp], _i,
                                     "tests/test_aux_loss_gpu.py"),
    "pct_sigmoid_focal_strided_forward_f32": ([_vp, _vp] + [_i] * 7 + [ctypes.c_float] + [_vp] * 4, _i,
                                              "tests/test_aux_loss_gpu.py"),
    "pct_sigmoid_focal_strided_backward_f32": ([_vp, _vp, _i, _vp, _vp] + [_i] * 6 + [ctypes.c_float, _vp, _vp], _i,
                                               "tests/test_aux_loss_gpu.py"),
}

# Entry point of the split-operand cross-attention for any key count (include/pctrans_hip_xattn.h; pctrans_amd/ragged_attention.py,
# reached with CrossAttentionLayer.ragged_keys = "hip").  A table of its own, as the losses': name -> (argtypes, restype, the
# test module that checks the entry -- against pct_masked_attention_bf16 on the concatenated operands: the outputs are the same bits)
XATTN_SYMBOLS = {
    "pct_cross_attention_ragged_bf16": ([_vp] * 6 + [_i, _vp] + [_i] * 4 + [ctypes.c_float, _vp, _vp], _i,
                                        "tests/test_ragged_attention_gpu.py"),
}

# Entry points of the same cross-attention with the keys divided over several workgroups and a combine launch
# (include/pctrans_hip_xattn_split.h; pctrans_amd/split_key_attention.py, reached with CrossAttentionLayer.split_keys = "hip").  A
# table of its own, as the ragged entry's: name -> (argtypes, restype, the test module that checks the entry against that entry
# and against float64)
XATTN_SPLIT_SYMBOLS = {
    "pct_cross_attention_split_keys_workspace": ([_i] * 4, ctypes.c_longlong, "tests/test_split_key_attention_gpu.py"),
    "pct_cross_attention_split_keys_bf16": ([_vp] * 6 + [_i, _vp] + [_i] * 4 + [ctypes.c_float, _i, _vp, ctypes.c_longlong, _vp, _vp],
                                            _i, "tests/test_split_key_attention_gpu.py"),
}

# Entry point of the small-object merging of label maps (include/pctrans_hip_merge.h; pctrans_amd/label_merge.py:
# merge_small_objects, MaskFormer.test_labels).  A table of its own, as the metrics': name -> (argtypes, restype, the test module
# that checks the entry -- against the table-based restatement of the reference's merge_func: the outputs are exact)
MERGE_SYMBOLS = {
    "pct_label_merge_small": ([_vp, _i, _vp, _i, _i, _i, _vp, _i] + [_vp] * 10, _i, "tests/test_label_merge_gpu.py"),
}

# Entry points of the decoder's attention in fp32 evaluation (include/pctrans_hip_attn_eval.h; pctrans_amd/attention_eval.py,
# reached with CrossAttentionLayer.attn_eval / SelfAttentionLayer.attn_eval = "hip").  A table of its own, as the merge's:
# name -> (argtypes, restype, the test module that checks the entry -- against the training forwards, bit for bit, and float64)
ATTN_EVAL_SYMBOLS = {
    "pct_cross_attention_eval_f32": ([_vp] * 7 + [_i] * 4 + [ctypes.c_float, _vp, _vp], _i, "tests/test_attention_eval_gpu.py"),
    "pct_self_attention_eval_f32": ([_vp] * 5 + [_i] * 3 + [ctypes.c_float, _vp, _vp], _i, "tests/test_attention_eval_gpu.py"),
}


class PctransLibraryError(RuntimeError):
    pass


def lib():
    """Load (once) and return the HIP library.  No fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PctransLibraryError(
            "libpctrans_hip.so not found at %s -- build it with `make -C pctrans_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`).  "
            "pctrans_amd has no CPU / eager fallback for device tensors." % LIB_PATH)
    l = ctypes.CDLL(LIB_PATH)
    for name, (argtypes, restype) in list(SYMBOLS.items()) + [
            (k, v[:2]) for k, v in list(OPT_IN_SYMBOLS.items()) + list(POST_SYMBOLS.items()) + list(SEG_SYMBOLS.items())
            + list(FPN_SYMBOLS.items()) + list(ATTN_TRAIN_SYMBOLS.items()) + list(REID_SYMBOLS.items()) + list(TARGETS_SYMBOLS.items())
            + list(MSDA_TRAIN_SYMBOLS.items()) + list(REID_QUERY_SYMBOLS.items()) + list(METRICS_SYMBOLS.items())
            + list(SELF_ATTN_TRAIN_SYMBOLS.items()) + list(AUX_LOSS_SYMBOLS.items()) + list(XATTN_SYMBOLS.items())
            + list(XATTN_SPLIT_SYMBOLS.items()) + list(MERGE_SYMBOLS.items()) + list(ATTN_EVAL_SYMBOLS.items())
            + list(ATTN_TRAIN_SPLIT_SYMBOLS.items())]:
        try:
            fn = getattr(l, name)
        except AttributeError as e:
            raise PctransLibraryError("libpctrans_hip.so does not export %s (stale build?)" % name) from e
        fn.argtypes = argtypes
        fn.restype = restype
    v = l.pct_abi_version()
    if v != ABI_VERSION:
        raise PctransLibraryError("libpctrans_hip.so ABI version %d, expected %d -- rebuild" % (v, ABI_VERSION))
    _lib = l
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().pct_error_string(code).decode()
        raise RuntimeError("%s failed: %s (code %d)" % (what, msg, code))


def env_switch(name, default="torch"):
    """Process default of an opt-in device path: the environment variable `name` = hip | torch, `default` where it is unset or
    empty.  Every module's `default()` is this."""
    v = os.environ.get(name) or default
    if v not in ("hip", "torch"):
        raise RuntimeError("%s must be 'hip' or 'torch', got %r" % (name, v))
    return v


def chunk_plan(pixels, per_pass, max_chunks):
    """(passes of `per_pass` pixels per chunk, chunks of an image): csrc/launchers.hpp's chunk_plan, for the workspace sizes."""
    subs = -(-pixels // per_pass)
    passes = -(-subs // max_chunks)
    return passes, -(-subs // passes)


_PREPARED = set()


def prepare_device(device):
    """Once per device: allocate the library's per-device pools now (include/pctrans_hip.h: pct_prepare_device), unless a
    stream capture is under way (the pools are then allocated by the first un-captured launch, as before)."""
    import torch
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx in _PREPARED:
        return
    if torch.cuda.is_current_stream_capturing():
        return
    with torch.cuda.device(idx):
        check(lib().pct_prepare_device(), "prepare_device")
    _PREPARED.add(idx)
