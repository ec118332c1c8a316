"""ctypes binding of libta3n_hip.so (include/ta3n_hip.h).

The library is loaded on first use.  If it has not been built the call raises -
there is no CPU or eager-PyTorch fallback for the product path.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, List, Optional, Tuple

# torch bundles its own libamdhip64; it must be in the process BEFORE libta3n_hip.so is
# dlopen'ed so both resolve to ONE HIP runtime (otherwise the second runtime sees no device).
import torch  # noqa: F401

_LIB: Optional[C.CDLL] = None
LIB_PATH = os.path.join(os.environ.get("TA3N_LIBDIR") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib"), "libta3n_hip.so")

FLAG_ADV_RELATION = 1 << 0
FLAG_ADV_VIDEO = 1 << 1
FLAG_ADV_FRAME = 1 << 2
FLAG_ATTN_ENTROPY = 1 << 3
FLAG_TRANS_ATTN = 1 << 4
FLAG_MCD = 1 << 5              # ens_DA 'MCD': second video classifier (regions Y2 / gY2); unfused entry points
FLAG_FEATURE_GRADS = 1 << 6    # backward also takes a gradient at the pooled video feature (region gV_ext): dis_DA DAN / JAN
FLAG_BN_SHARED = 1 << 7        # use_bn AdaBN / AutoDIAL: BatchNorm1d per domain behind the shared frame FC (regions Z0, bn_batch, bn_run)
FLAG_BF16_MFMA = 1 << 8
FLAG_BF16_STORE = 1 << 9
FLAG_F32_SPLIT = 1 << 10       # fp32-grade contractions as three bf16 MFMAs on operands split hi + lo in registers ("bf16x3")
FLAG_FRAME_ATTN = 1 << 11      # use_attn_frame TransAttn: frame features scaled by 1 + (1 - H(frame-discriminator softmax)) in front of the TRN (regions F1a, attn_frame); unfused entry points
FLAG_CLASS_WEIGHTS = 1 << 12   # --weighted_class_loss: every class CE weighted per class (region class_w, written by the caller); single rank
FLAG_TARGET_LABELS = 1 << 13   # --use_target Sv: the class CE over the valid rows of both halves, target labels in region "labels"[Bs:]; single rank
FLAG_TARGET_ENTROPY = 1 << 14  # --add_loss_DA target_entropy: gamma * mean entropy of the valid target rows' class softmax; exclusive with FLAG_ATTN_ENTROPY
FLAG_GENERAL_ATTN = 1 << 15   # use_attn general: relation weights = softmax over the relations of a learned layer's scores (parameters attn_layer.0 / .2; regions Ua, gUa, gs); unfused entry points, single rank
FLAG_UNSHARED = 1 << 16       # share_params N: the target rows' own first frame layer and video classifier (parameters fc_*_target); unfused entry points, single rank
FLAG_SCORE_ONLY = 1 << 17     # a score-only plan: the eval-mode forward to the class logits on the training plan's parameter layout, scored by ta3n_score (ta3n_amd.scoring.Scorer)
FLAG_TRAIN_METERS = 1 << 18   # training meters: one more launch per step accumulates loss sums, Prec@1/5 and domain accuracy in regions meter_counts / meter_sums
AGG_TRN_M, AGG_AVGPOOL, AGG_RNN = 0, 1, 2      # AGG_RNN: slot max-pooling + one LSTM / GRU layer (rnn_cell, n_ts)
AGG_TEMCONV = 4                                 # the 3-tap filter tcl_3_1 over the segments + ReLU + mean (3 would be the reference's 'trn', which it cannot run)
RNN_CELLS = {"LSTM": 0, "GRU": 1}

# every symbol include/ta3n_hip.h declares (tests check the export list)
SYMBOLS = [
    "ta3n_num_relation_tuples", "ta3n_relation_table", "ta3n_segment_indices", "ta3n_rnn_slots", "ta3n_gather_segments", "ta3n_plan_create",
    "ta3n_plan_destroy", "ta3n_num_params", "ta3n_param_info", "ta3n_param_floats", "ta3n_live_param_floats",
    "ta3n_workspace_floats", "ta3n_ws_offset", "ta3n_ws_size", "ta3n_plan_describe", "ta3n_set_hyper",
    "ta3n_init_workspace", "ta3n_forward", "ta3n_loss", "ta3n_backward", "ta3n_has_fused_step", "ta3n_train_step", "ta3n_eval_metrics", "ta3n_score",
    "ta3n_sgd_step", "ta3n_sgd_step_fused", "ta3n_sgd_range", "ta3n_train_step_join", "ta3n_train_step_range", "ta3n_refresh_bf16", "ta3n_sgd_step_next", "ta3n_gather_segments_into", "ta3n_has_pipelined_step", "ta3n_train_step_after_update", "ta3n_num_phases",
    "ta3n_adam_scalars", "ta3n_adam_range", "ta3n_adam_step_next", "ta3n_train_steps_adam",
    "ta3n_debug_arrays", "ta3n_debug_struct_sizes", "ta3n_time_phases", "ta3n_time_update_launches", "ta3n_last_error", "ta3n_version",
    "ta3n_comm_unique_id", "ta3n_comm_create", "ta3n_comm_destroy", "ta3n_comm_world", "ta3n_all_reduce_sum", "ta3n_train_step_ddp",
    "ta3n_gather_segments_bf16_into", "ta3n_train_steps", "ta3n_train_steps_multi", "ta3n_chain_status", "ta3n_debug_waits",
    "ta3n_peer_create", "ta3n_peer_handle", "ta3n_peer_connect", "ta3n_peer_all_reduce_sum", "ta3n_peer_status", "ta3n_peer_destroy",
    "ta3n_comm_attach_peer", "ta3n_has_fused_update", "ta3n_train_steps_fused_update",
    "ta3n_gaussian_kernel_scratch_floats", "ta3n_gaussian_kernel", "ta3n_mmd_rowdiff", "ta3n_discrepancy_scratch_floats", "ta3n_discrepancy",
    "ta3n_mcd_source_loss", "ta3n_mcd_second_loss",
    "ta3n_set_heads_waves", "ta3n_get_heads_waves",
    "ta3n_num_live_ranges", "ta3n_live_range", "ta3n_sgd_live",
    "ta3n_shard_ranges", "ta3n_shard_sumsq", "ta3n_sgd_shard", "ta3n_shard_reduce_scatter", "ta3n_sharded_update", "ta3n_train_steps_sharded",
    "ta3n_sample_segments", "ta3n_gather_segments_sampled", "ta3n_gather_segments_bf16", "ta3n_gather_segments_sampled_into",
    "ta3n_gather_segments_bf16_sampled_into",
    "ta3n_meters_reset",
]
SAMPLERS = {"test": 0, "val": 1, "train": 2}      # TA3N_SAMPLER_* (TSNDataSet._get_test_indices / _get_val_indices / _sample_indices)


class Config(C.Structure):
    _fields_ = [("batch_source", C.c_int32), ("batch_target", C.c_int32), ("num_segments", C.c_int32),
                ("feature_dim", C.c_int32), ("fc_dim", C.c_int32), ("num_bottleneck", C.c_int32),
                ("num_class", C.c_int32), ("flags", C.c_uint32), ("tile_config", C.c_int32),
                ("phase_tiles", C.c_int32 * 16), ("xcd_aware", C.c_int32), ("aggregation", C.c_int32),
                ("wgrads_late", C.c_int32), ("chain", C.c_int32), ("cost_model", C.c_int32), ("split_k", C.c_int32),
                ("shared_fc_layers", C.c_int32),      # --add_fc (0 / 1: one shared layer)
                ("layout_flags", C.c_uint32),         # 0, or the flags of the configuration whose flat parameter layout this plan adopts
                ("rnn_cell", C.c_int32), ("n_ts", C.c_int32)]      # AGG_RNN: 0 LSTM / 1 GRU; recurrent steps (0: 5)


class Hyper(C.Structure):
    _fields_ = [("beta", C.c_float * 3), ("gamma", C.c_float), ("lr", C.c_float), ("momentum", C.c_float),
                ("weight_decay", C.c_float), ("clip", C.c_float), ("p_drop_i", C.c_float), ("p_drop_v", C.c_float),
                ("seed_i", C.c_uint32), ("seed_v", C.c_uint32), ("inv_n_cls", C.c_float), ("inv_n_rel", C.c_float),
                ("inv_n_vid", C.c_float), ("inv_n_frm", C.c_float), ("inv_n_ent", C.c_float),
                ("valid_source", C.c_int32), ("valid_target", C.c_int32), ("train", C.c_int32),
                ("reverse", C.c_int32), ("mu", C.c_float), ("bn_eval_target", C.c_int32), ("class_w_off", C.c_int32), ("dom_k", C.c_float * 2)]


class Feed(C.Structure):
    """ta3n_feed (include/ta3n_hip.h): device-side batch assembly of a multi-step call."""
    _fields_ = [("store", C.c_void_p), ("bf16", C.c_int32), ("ids_per_step", C.c_int32), ("first_row", C.c_void_p),
                ("num_frames", C.c_void_p), ("labels", C.c_void_p), ("video_ids", C.c_void_p),
                ("sampler", C.c_int32), ("seed", C.c_uint32), ("step0", C.c_uint32)]      # all zero: the test-mode sampler


class StepsJob(C.Structure):
    """ta3n_steps_job (include/ta3n_hip.h): the argument list of one ta3n_train_steps call, as an element of ta3n_train_steps_multi."""
    _fields_ = [("plan", C.c_void_p), ("x", C.c_void_p), ("params", C.c_void_p), ("grads", C.c_void_p), ("momentum", C.c_void_p),
                ("ws", C.c_void_p), ("fused_norm", C.c_int32), ("lr_pending", C.c_float), ("momentum_coef", C.c_float),
                ("weight_decay", C.c_float), ("clip", C.c_float), ("hypers", C.POINTER(Hyper)), ("source", C.POINTER(Feed)),
                ("target", C.POINTER(Feed)), ("comm", C.c_void_p), ("scratch_bf16", C.c_void_p), ("stream", C.c_void_p)]


class Ta3nError(RuntimeError):
    pass


def has_experiments() -> bool:
    """True when the loaded library was built with -DTA3N_EXPERIMENTS=1 (the measured-and-rejected step variants: chained launches,
    split-K tiles, the optimiser inside the gradient tiles, the tall four-wave tiles; `pytest -m gpu_ab`)."""
    return lib().ta3n_version().decode().endswith("+experiments")


def lib() -> C.CDLL:
    """Load the HIP library (once).  Raises if it is missing: build it with
    `python -m ta3n_amd.build` (hipcc --offload-arch=gfx950)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise Ta3nError(f"{LIB_PATH} not found: the HIP extension is required (python -m ta3n_amd.build); "
                        "there is no CPU fallback")
    # The binary must be the one these sources build: the hash of csrc/ + include/ stored beside it at link time (ta3n_amd/build.py)
    # against the hash of the tree that is loading it.  A stale or hand-placed library fails here, loudly (TA3N_ALLOW_STALE_LIB=1: A/B
    # runs of an older build directory on purpose).
    try:
        from .build import source_hash
        with open(os.path.join(os.path.dirname(LIB_PATH), ".source_hash")) as fh:
            linked_from = fh.read().strip()
        if linked_from != source_hash() and os.environ.get("TA3N_ALLOW_STALE_LIB") != "1":
            raise Ta3nError(f"{LIB_PATH} was linked from sources {linked_from}, this tree is {source_hash()}: rebuild "
                            "(python -m ta3n_amd.build), or TA3N_ALLOW_STALE_LIB=1 to load it anyway")
    except OSError:
        pass                              # (a library without a recorded hash: built by hand; nothing to compare)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.ta3n_num_relation_tuples.argtypes = [C.c_int]
    L.ta3n_relation_table.argtypes = [C.c_int, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.ta3n_segment_indices.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(i64)]
    L.ta3n_rnn_slots.argtypes = [C.c_int, C.c_int, C.POINTER(i32), C.POINTER(i32)]
    L.ta3n_gather_segments.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    key = [C.c_int, C.c_uint32, C.c_uint32]      # sampler, seed, step
    L.ta3n_sample_segments.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(i64)]
    L.ta3n_gather_segments_sampled.argtypes = L.ta3n_gather_segments.argtypes + key
    L.ta3n_gather_segments_bf16.argtypes = L.ta3n_gather_segments.argtypes + key
    L.ta3n_plan_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.ta3n_plan_destroy.argtypes = [vp]
    L.ta3n_plan_destroy.restype = None
    L.ta3n_num_params.argtypes = [vp]
    L.ta3n_param_info.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32),
                                  C.POINTER(i32)]
    for fn in ("ta3n_param_floats", "ta3n_live_param_floats", "ta3n_workspace_floats"):
        getattr(L, fn).argtypes = [vp]
        getattr(L, fn).restype = i64
    for fn in ("ta3n_ws_offset", "ta3n_ws_size"):
        getattr(L, fn).argtypes = [vp, C.c_char_p]
        getattr(L, fn).restype = i64
    L.ta3n_plan_describe.argtypes = [vp, C.c_char_p, i64]
    L.ta3n_plan_describe.restype = i64
    L.ta3n_set_hyper.argtypes = [vp, vp, C.POINTER(Hyper), vp]
    L.ta3n_init_workspace.argtypes = [vp, vp, vp]
    L.ta3n_forward.argtypes = [vp, vp, vp, vp, vp]
    L.ta3n_loss.argtypes = [vp, vp, vp]
    L.ta3n_backward.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ta3n_eval_metrics.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.ta3n_score.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp]
    L.ta3n_meters_reset.argtypes = [vp, vp, vp]
    L.ta3n_has_fused_step.argtypes = [vp]
    L.ta3n_train_step.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ta3n_sgd_step.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ta3n_sgd_step_fused.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ta3n_sgd_range.argtypes = [vp, vp, vp, vp, vp, i64, i64, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, vp]
    L.ta3n_train_step_join.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.ta3n_num_live_ranges.argtypes = [vp]
    L.ta3n_live_range.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(i64)]
    L.ta3n_sgd_live.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, vp]
    L.ta3n_train_step_range.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp]
    L.ta3n_refresh_bf16.argtypes = [vp, vp, vp, vp, vp]
    L.ta3n_has_pipelined_step.argtypes = [vp]
    L.ta3n_train_step_after_update.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp]
    L.ta3n_train_steps.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(Hyper), C.c_int,
                                   C.POINTER(Feed), C.POINTER(Feed), vp, vp, vp]
    L.ta3n_train_steps_multi.argtypes = [C.POINTER(StepsJob), C.c_int, C.c_int]
    L.ta3n_has_fused_update.argtypes = [vp]
    L.ta3n_shard_ranges.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64)]
    L.ta3n_shard_sumsq.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp]
    L.ta3n_sgd_shard.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(Hyper), vp]
    L.ta3n_shard_reduce_scatter.argtypes = [vp, vp, vp, vp, vp]
    L.ta3n_sharded_update.argtypes = [vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(Hyper), vp]
    L.ta3n_train_steps_sharded.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(Hyper), C.c_int,
                                           C.POINTER(Feed), C.POINTER(Feed), vp, vp, vp]
    L.ta3n_train_steps_fused_update.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.POINTER(Hyper), C.c_int,
                                                C.POINTER(Feed), C.POINTER(Feed), vp]
    L.ta3n_gather_segments_into.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.ta3n_gather_segments_bf16_into.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.ta3n_gather_segments_sampled_into.argtypes = L.ta3n_gather_segments_into.argtypes + key
    L.ta3n_gather_segments_bf16_sampled_into.argtypes = L.ta3n_gather_segments_into.argtypes + key
    L.ta3n_sgd_step_next.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp]
    L.ta3n_num_phases.argtypes = [vp, C.c_int]
    f32, f64 = C.c_float, C.c_double
    L.ta3n_adam_scalars.argtypes = [i64, f32, f64, f64, C.POINTER(f32), C.POINTER(f32)]
    L.ta3n_adam_range.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, C.c_int, f32, f64, f64, f32, f32, f32, i64, vp]
    L.ta3n_adam_step_next.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, f32, f64, f64, f32, f32, f32, i64, C.POINTER(Hyper), vp]
    L.ta3n_train_steps_adam.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, f32, f64, f64, f32, f32, f32, i64, C.POINTER(Hyper), C.c_int,
                                        C.POINTER(Feed), C.POINTER(Feed), vp]
    L.ta3n_time_update_launches.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, vp, C.c_int,
                                            C.POINTER(C.c_float)]
    L.ta3n_time_phases.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_float), C.POINTER(i32), C.POINTER(i32),
                                   C.c_int]
    L.ta3n_debug_arrays.argtypes = [vp] + [C.POINTER(vp), C.POINTER(i64)] * 3 + [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.ta3n_debug_struct_sizes.argtypes = [C.POINTER(i32)] * 5
    L.ta3n_debug_waits.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.ta3n_chain_status.argtypes = [vp, vp, vp]
    L.ta3n_comm_unique_id.argtypes = [C.c_char_p]
    L.ta3n_comm_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    L.ta3n_comm_destroy.argtypes = [vp]
    L.ta3n_comm_destroy.restype = None
    L.ta3n_comm_world.argtypes = [vp]
    L.ta3n_all_reduce_sum.argtypes = [vp, vp, i64, vp, vp]
    L.ta3n_train_step_ddp.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ta3n_peer_create.argtypes = [C.c_int, C.c_int, i64, C.c_int, C.POINTER(vp)]
    L.ta3n_peer_handle.argtypes = [vp, C.c_char_p]
    L.ta3n_peer_connect.argtypes = [vp, C.c_char_p]
    L.ta3n_peer_all_reduce_sum.argtypes = [vp, vp, i64, vp]
    L.ta3n_peer_status.argtypes = [vp, vp]
    L.ta3n_peer_destroy.argtypes = [vp]
    L.ta3n_peer_destroy.restype = None
    L.ta3n_comm_attach_peer.argtypes = [vp, vp]
    L.ta3n_gaussian_kernel_scratch_floats.argtypes = [C.c_int]
    L.ta3n_gaussian_kernel_scratch_floats.restype = i64
    L.ta3n_gaussian_kernel.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, vp, vp, vp, vp]
    L.ta3n_mmd_rowdiff.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, vp, vp]
    L.ta3n_mcd_source_loss.argtypes = [vp, vp, vp, vp, vp]
    L.ta3n_mcd_second_loss.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp]
    L.ta3n_discrepancy_scratch_floats.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.ta3n_discrepancy_scratch_floats.restype = i64
    L.ta3n_discrepancy.argtypes = [vp, i64, C.c_int, i64, C.c_int, i64, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_float, vp, i64, vp, vp]
    if hasattr(L, "ta3n_set_heads_waves"):      # (absent from an older build directory loaded on purpose: TA3N_ALLOW_STALE_LIB=1, A/B runs)
        L.ta3n_set_heads_waves.argtypes = [C.c_int]
        L.ta3n_get_heads_waves.argtypes = [vp]
    L.ta3n_last_error.restype = C.c_char_p
    L.ta3n_version.restype = C.c_char_p
    _LIB = L
    return L


def check(rc: int, what: str = "") -> int:
    if rc < 0:
        msg = lib().ta3n_last_error().decode()
        if rc == -1:
            raise ValueError(f"{what}: {msg}")        # the reference raises ValueError for bad configs (models.py:137, 562)
        raise Ta3nError(f"{what}: {msg} (status {rc})")
    return rc


def relation_table(num_frames: int) -> List[List[Tuple[int, ...]]]:
    """Selected frame tuples per scale, scale T first (reference TRNmodule.py:30-41, 60, 68-71)."""
    L = lib()
    n = check(L.ta3n_num_relation_tuples(num_frames), "ta3n_num_relation_tuples")
    tup = (C.c_int32 * (n * num_frames))()
    sl = (C.c_int32 * n)()
    sid = (C.c_int32 * n)()
    check(L.ta3n_relation_table(num_frames, tup, sl, sid), "ta3n_relation_table")
    out: List[List[Tuple[int, ...]]] = [[] for _ in range(num_frames - 1)]
    for r in range(n):
        out[sid[r]].append(tuple(tup[r * num_frames + j] for j in range(sl[r])))
    return out


def segment_indices(num_frames: int, num_segments: int, new_length: int = 1) -> List[int]:
    """TSNDataSet._get_test_indices (reference dataset.py:103-116); 1-based."""
    L = lib()
    out = (C.c_int64 * num_segments)()
    check(L.ta3n_segment_indices(num_frames, num_segments, new_length, out), "ta3n_segment_indices")
    return list(out)


def sampler_code(sampler) -> int:
    """TA3N_SAMPLER_* of a sampler's name ("test" / "val" / "train"; a code passes through)."""
    if isinstance(sampler, str) and sampler in SAMPLERS:
        return SAMPLERS[sampler]
    if not isinstance(sampler, (str, bool)) and sampler in SAMPLERS.values():
        return int(sampler)
    raise ValueError(f"sampler must be one of 'test', 'val', 'train', not {sampler!r}")


def sample_segments(sampler, num_frames: int, num_segments: int, seed: int = 0, step: int = 0, slot: int = 0) -> List[int]:
    """The 1-based frame ids a device gather with (sampler, seed, step) selects for the video in position `slot` of its call
    (ta3n_sample_segments: the host side of the kernels' own rule, new_length 1)."""
    L = lib()
    out = (C.c_int64 * num_segments)()
    check(L.ta3n_sample_segments(sampler_code(sampler), num_frames, num_segments, seed & 0xFFFFFFFF, step & 0xFFFFFFFF, slot & 0xFFFFFFFF, out),
          "ta3n_sample_segments")
    return list(out)


def rnn_slots(num_segments: int, n_ts: int) -> Tuple[int, List[int]]:
    """(len_ts, frame read by each of the len_ts * n_ts pooling slots) of the recurrent aggregator (reference models.py:397-409);
    raises ValueError where the reference fails (len_ts == 0)."""
    L = lib()
    len_ts = C.c_int32()
    frames = (C.c_int32 * 256)()
    check(L.ta3n_rnn_slots(num_segments, n_ts, C.byref(len_ts), frames), "ta3n_rnn_slots")
    return len_ts.value, list(frames[:len_ts.value * n_ts])


# ---- training meters (TA3N_FLAG_TRAIN_METERS; include/ta3n_hip.h) ----
METER_WORDS = 32          # int32 words of region "meter_counts"
METER_SUMS = 8            # float64 words of region "meter_sums", 64 floats behind "meter_counts"
METER_FLOATS = 64 + 2 * METER_SUMS      # floats from the start of "meter_counts" to the end of "meter_sums": one copy reads both
METER_LEVELS = ("rel", "vid", "frm")
METER_LOSSES = ("loss", "loss_c", "loss_adv_rel", "loss_adv_vid", "loss_adv_frm", "loss_e")


def read_meters(plan: "Plan", ws: "torch.Tensor"):
    """Both meter regions of a flagged plan's workspace with ONE device-to-host copy: (int64 counts [32], float64 sums [8])."""
    o, _ = plan.region("meter_counts")
    o2, _ = plan.region("meter_sums")
    assert o2 == o + 64 and o2 % 2 == 0, (o, o2)
    raw = ws[o:o + METER_FLOATS].cpu()
    counts = raw[:METER_WORDS].view(torch.int32).to(torch.int64)
    sums = raw[64:64 + 2 * METER_SUMS].view(torch.float64).clone()
    return counts, sums


def _pct(hit: int, n: int) -> float:
    return 100.0 * hit / n if n else 0.0


def decode_meters(counts, sums, world: int = 1) -> Dict[str, object]:
    """The words of the two regions as the dict TrainEngine.meters() returns: per-step loss means, accuracies in percent, raw counts.
    world > 1: the words are the SUM over that many ranks - every rank counted every step, and a rank's loss slots are its shard's share
    of the job's mean: the step counts are divided by world (a step some rank found non-finite counts as one), the sums are the job's."""
    c = [int(v) for v in counts]
    s = [float(v) for v in sums]
    finite = (c[0] - c[1]) / world
    out: Dict[str, object] = {"steps": c[0] // world, "nonfinite_steps": -(-c[1] // world)}
    for i, k in enumerate(METER_LOSSES):
        out[k] = s[i] / finite if finite else 0.0
    out.update(prec1=_pct(c[3], c[2]), prec5=_pct(c[4], c[2]), prec1_last=_pct(c[6], c[5]), prec5_last=_pct(c[7], c[5]))
    dom = {lv: tuple(c[8 + 4 * l + 2 * d: 8 + 4 * l + 2 * d + 2] for d in (0, 1)) for l, lv in enumerate(METER_LEVELS)}
    out["acc_domain"] = {lv: tuple(_pct(hit, n) for n, hit in dom[lv]) for lv in METER_LEVELS}
    out["counts"] = {"source_rows": c[2], "top1": c[3], "top5": c[4], "last_source_rows": c[5], "last_top1": c[6], "last_top5": c[7],
                     "domain": {lv: {"source": tuple(dom[lv][0]), "target": tuple(dom[lv][1])} for lv in METER_LEVELS}}      # (rows, correct)
    out["loss_sums"] = dict(zip(METER_LOSSES, s[:6]))
    return out


class Plan:
    """Owns a ta3n_plan handle and caches its layout tables."""

    def __init__(self, batch_source: int, batch_target: int, num_segments: int, feature_dim: int, fc_dim: int,
                 num_class: int, flags: int, num_bottleneck: int = 256, tile_config: int = 0,
                 phase_tiles: Optional[List[int]] = None, xcd_aware: int = 0, aggregation: int = 0, wgrads_late: int = 0,
                 chain: int = 0, cost_model: int = 0, split_k: int = 0, shared_fc_layers: int = 0, layout_flags: int = 0,
                 rnn_cell: int = 0, n_ts: int = 0):
        L = lib()
        self.cfg = Config(batch_source, batch_target, num_segments, feature_dim, fc_dim, num_bottleneck, num_class,
                          flags, tile_config)
        for i, t in enumerate((phase_tiles or [])[:16]):      # (launches past the 16th mirror an earlier one or use tile_config)
            self.cfg.phase_tiles[i] = int(t)
        self.cfg.xcd_aware = int(xcd_aware)
        self.cfg.aggregation = int(aggregation)       # AGG_TRN_M / AGG_AVGPOOL
        self.cfg.wgrads_late = int(wgrads_late)
        self.cfg.chain = int(chain)
        self.cfg.cost_model = int(cost_model)
        self.cfg.split_k = int(split_k)
        self.cfg.shared_fc_layers = int(shared_fc_layers)      # --add_fc (models.py:145-153)
        self.cfg.layout_flags = int(layout_flags)              # the parameter layout of the plan these flags would give (0: its own)
        self.cfg.rnn_cell = int(rnn_cell)                      # AGG_RNN: 0 LSTM, 1 GRU
        self.cfg.n_ts = int(n_ts)                              # AGG_RNN: recurrent steps (0: 5)
        h = C.c_void_p()
        check(L.ta3n_plan_create(C.byref(self.cfg), C.byref(h)), "ta3n_plan_create")
        self.handle = h
        self._L = L
        n = L.ta3n_num_params(h)
        self.params: List[Tuple[str, int, Tuple[int, ...], bool]] = []
        for i in range(n):
            name = C.c_char_p(); off = C.c_int64(); r = C.c_int32(); c = C.c_int32(); live = C.c_int32()
            check(L.ta3n_param_info(h, i, C.byref(name), C.byref(off), C.byref(r), C.byref(c), C.byref(live)))
            shape = (r.value, c.value) if c.value else (r.value,)
            self.params.append((name.value.decode(), off.value, shape, bool(live.value)))
        self.param_floats = L.ta3n_param_floats(h)
        self.live_floats = L.ta3n_live_param_floats(h)
        self.ws_floats = L.ta3n_workspace_floats(h)
        n = L.ta3n_plan_describe(h, None, 0)
        buf = C.create_string_buffer(n + 1)
        L.ta3n_plan_describe(h, buf, n + 1)
        self.description = json.loads(buf.value.decode())
        self.regions: Dict[str, Tuple[int, int]] = {k: tuple(v) for k, v in self.description["regions"].items()}
        self.has_fused_step = L.ta3n_has_fused_step(h) == 1
        self.has_fused_update = L.ta3n_has_fused_update(h) == 1
        # the float ranges of the flat buffer that hold the live parameters (one, the live prefix, without layout_flags)
        self.live_ranges: List[Tuple[int, int]] = []
        for i in range(L.ta3n_num_live_ranges(h)):
            b = C.c_int64(); e = C.c_int64()
            check(L.ta3n_live_range(h, i, C.byref(b), C.byref(e)), "ta3n_live_range")
            self.live_ranges.append((b.value, e.value))

    def region(self, name: str) -> Tuple[int, int]:
        return self.regions[name]

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._L.ta3n_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass
