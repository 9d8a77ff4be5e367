"""ctypes binding of `libbesskge_hip.so` (C ABI: include/besskge_hip.h).

This is the only place the Python side touches the native library.  Tensors
are validated here (device, dtype, contiguity, shapes) so that a kernel never
sees operand shapes its grid does not assume; then raw device pointers and
PyTorch's current HIP stream are handed over.  PyTorch is used for device
memory and streams only.

There is deliberately no CPU fallback: every wrapper raises if a tensor is not
on a CUDA/HIP device or if the library is missing.
"""

import contextlib
import ctypes
import pathlib
import sys
import threading
from typing import Any, List, Optional, Sequence, Tuple

import torch

LIB_NAME = "libbesskge_hip.so"
ABI_VERSION = 3

TRANSE, ROTATE, DISTMULT, COMPLEX, AFFINE, BOXE = 0, 1, 2, 3, 4, 5
F32, F16 = 0, 1
CORRUPT_HEAD, CORRUPT_TAIL = 0, 1
LOSS_LOGSIGMOID, LOSS_MARGIN, LOSS_SSCE = 0, 1, 2
BAD_NEGATIVE_SCORE = -50000.0

_c_i32p = ctypes.POINTER(ctypes.c_int32)
_c_f32p = ctypes.POINTER(ctypes.c_float)
_c_u8p = ctypes.POINTER(ctypes.c_uint8)
_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_RETURNS_I64 = ("bess_neg_score_shared_workspace", "bess_neg_score_shared_bwd_workspace",
                "bess_neg_score_shared_fwd_counts_workspace", "bess_neg_score_shared_fwd_pairs_workspace",
                "bess_neg_score_table_fwd_counts_workspace", "bess_neg_score_table_fwd_pairs_workspace",
                "bess_neg_score_shared_fwd_lse_workspace", "bess_neg_score_shared_bwd_softmax_workspace")  # every other entry returns an int status
_i32 = ctypes.c_int32
_f32 = ctypes.c_float


class ModelDesc(ctypes.Structure):
    """struct bess_model_desc"""

    _fields_ = [
        ("scorer", _i32),
        ("norm_p", _i32),
        ("dtype", _i32),
        ("width", _i32),
        ("rel_width", _i32),
        ("reserved", _i32 * 3),
    ]


class LossDesc(ctypes.Structure):
    """struct bess_loss_desc"""

    _fields_ = [
        ("kind", _i32),
        ("adversarial", _i32),
        ("margin", _f32),
        ("adversarial_scale", _f32),
        ("loss_scale", _f32),
        ("ssce_shift", _f32),
        ("reserved", _i32 * 2),
    ]


class OptDesc(ctypes.Structure):
    """struct bess_opt_desc"""

    _fields_ = [
        ("kind", _i32),
        ("step", _i32),
        ("lr", _f32),
        ("momentum", _f32),
        ("beta1", _f32),
        ("beta2", _f32),
        ("eps", _f32),
        ("weight_decay", _f32),
        ("step_ptr", _i64),
        ("slot_map", _i64),
    ]


OPT_SGD, OPT_ADAGRAD, OPT_ADAM = 0, 1, 2
FLAG_FP32_MATH = 1  # BESS_FLAG_FP32_MATH (ModelDesc.reserved[0] of the four native scorers)
FLAG_PREZEROED = 2  # BESS_FLAG_PREZEROED: the targets of bess_neg_score_shared_bwd are zero on entry
FLAG_DNEG_BY_ROW = 4  # BESS_FLAG_DNEG_BY_ROW: bess_neg_score_pertriple_bwd stores d_neg at row neg_idx[k] of a row-space matrix


class KillDesc(ctypes.Structure):
    """struct bess_kill_desc: K7 (mask / augment kill) applied with the scores"""

    _fields_ = [
        ("diag_step", _i32),
        ("ht", _i32),
        ("ppp", _i32),
        ("reserved", _i32),
        ("mask", _vp),
        ("mask_rows", _i64),
        ("mask_cols", _i64),
    ]


class Pcg64State(ctypes.Structure):
    """struct bess_pcg64_state"""

    _fields_ = [
        ("state_hi", ctypes.c_uint64),
        ("state_lo", ctypes.c_uint64),
        ("inc_hi", ctypes.c_uint64),
        ("inc_lo", ctypes.c_uint64),
        ("has_uint32", ctypes.c_uint32),
        ("uinteger", ctypes.c_uint32),
    ]


_PG = ctypes.POINTER(Pcg64State)

_MD = ctypes.POINTER(ModelDesc)
_LD = ctypes.POINTER(LossDesc)

# name -> argtypes; every function returns int
SIGNATURES = {
    "bess_version": [],
    "bess_last_error": [ctypes.c_char_p, ctypes.c_size_t],
    "bess_gather_rows": [_i32, _i32, _vp, _vp, _i64, _vp, _vp],
    "bess_score_triple_fwd": [_MD, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp],
    "bess_score_triple_bwd": [_MD, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "bess_query_fwd": [_MD, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp],
    "bess_query_bwd": [_MD, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp],
    "bess_query_triple_fwd": [_MD, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "bess_query_triple_bwd": [_MD, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    "bess_sparse_sgd_lists": [_i32, _i32, _vp, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64), _f32, _vp],
    "bess_sparse_sgd_lists_axpy": [_i32, _i32, _vp, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64), _f32,
                                   _vp, _vp, _i64, _f32, _vp],
    "bess_neg_score_pertriple_fwd": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp],
    "bess_neg_score_pertriple_bwd": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp],
    "bess_neg_score_shared_fwd": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp],
    "bess_neg_score_shared_workspace": [_MD, _i64, _i64],
    "bess_neg_score_shared_fwd_ws": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp],
    "bess_neg_score_shared_fwd_pruned": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp],
    "bess_neg_score_shared_fwd_counts_workspace": [_MD, _i64, _i64],
    "bess_neg_score_shared_fwd_counts": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _i64, _vp],
    "bess_neg_score_shared_fwd_pairs_workspace": [_MD, _i64, _i64],
    "bess_neg_score_shared_fwd_pairs": [_MD, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp],
    "bess_neg_score_shared_fwd_lse_workspace": [_MD, _i64, _i64],
    "bess_neg_score_shared_fwd_lse": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp],
    "bess_neg_score_shared_bwd_softmax_workspace": [_MD, _i64, _i64],
    "bess_neg_score_shared_bwd_softmax": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "bess_neg_score_table_fwd_counts_workspace": [_MD, _i64, _i64],
    "bess_neg_score_table_fwd_counts": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _i64, _vp],
    "bess_neg_score_table_fwd_pairs_workspace": [_MD, _i64, _i64],
    "bess_neg_score_table_fwd_pairs": [_MD, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp],
    "bess_topk_update_flagged": [_vp, _i64, _i64, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _vp],
    "bess_neg_score_shared_fwd_masked": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _i64, ctypes.POINTER(KillDesc), _vp, _i64, _vp],
    "bess_neg_score_shared_bwd": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp],
    "bess_neg_score_shared_bwd_workspace": [_MD, _i64, _i64],
    "bess_neg_score_shared_bwd_ws": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp],
    "bess_mask_scores": [_vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _i64, _vp],
    "bess_loss_fwd_bwd": [_LD, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp],
    "bess_loss_fwd_bwd_norm": [_LD, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp],
    "bess_loss_fwd_bwd_one_launch": [_LD, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "bess_loss_fwd_bwd_logq": [_LD, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64,
                               _i64, _i32, _f32, _vp],
    "bess_scatter_add_rows": [_vp, _i32, _vp, _vp, _i64, _f32, _vp],
    "bess_sparse_sgd": [_i32, _i32, _vp, _vp, _vp, _i64, _f32, _vp],
    "bess_dense_sgd": [_i32, _vp, _vp, _i64, _f32, _vp],
    "bess_segment_index_workspace": [_i64, ctypes.POINTER(ctypes.c_size_t)],
    "bess_build_segment_index": [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp, ctypes.c_size_t, _vp],
    "bess_pad_segments": [_vp, _vp, _i64, _vp, _i32, _vp],
    "bess_step_prologue": [_i32, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_uint32),
                           ctypes.POINTER(_i64), _i32, ctypes.POINTER(_vp), ctypes.POINTER(_i64), _i32, _vp, _vp, _vp, _vp,
                           _vp, _i64, _vp],
    "bess_neg_pertriple_grad_segments": [_MD, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _f32,
                                         _vp, _i64, _vp, _vp, _vp],
    "bess_apply_segments_sgd": [_i32, _i32, _vp, _vp, _vp, _i64, _vp, _f32, _vp],
    "bess_segment_sum_rows": [_i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp],
    "bess_topk_update": [_vp, _i64, _i64, _i64, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _i32, _vp],
    "bess_topk_update_excl": [_vp, _i64, _i64, _i64, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp],
    "bess_topk_update_flagged_excl": [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp],
    "bess_ranks_from_scores": [_vp, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _vp],
    "bess_ranks_from_indices": [_vp, _vp, _i64, _i64, _i32, _vp, _vp],
    "bess_apply_segments_opt": [ctypes.POINTER(OptDesc), _i32, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "bess_neg_pertriple_step_segments": [_MD, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64,
                                         _vp, _i64, _vp, _vp, ctypes.POINTER(OptDesc), _vp, _vp, _vp, _vp, _vp],
    "bess_map_extra_rows": [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp],
    "bess_assign_state_rows": [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp],
    "bess_coalesced_update": [ctypes.POINTER(OptDesc), _i32, _i32, _vp, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_i64),
                              _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "bess_coalesced_update_axpy": [ctypes.POINTER(OptDesc), _i32, _i32, _vp, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_i64),
                                   _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _f32, _vp],
    "bess_neg_pertriple_items": [_MD, _i64, _i64, ctypes.POINTER(ctypes.c_int32)],
    "bess_neg_pertriple_sweep": [_MD, _i64, _i64, ctypes.POINTER(ctypes.c_int32)],
    "bess_neg_score_pertriple_fwd_dq": [_MD, _LD, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp],
    "bess_neg_score_pertriple_fwd_dq_masked": [_MD, _LD, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp,
                                               _vp, _vp, _vp],
    "bess_neg_score_pertriple_fwd_partials": [_MD, _LD, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp],
    "bess_combine_dq_partials": [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp],
    "bess_normalize_rows": [_i32, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp],
    "bess_normalize_rows_bwd": [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp],
    "bess_sample_negatives": [_PG, _vp, _i64, _i32, _i32, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "bess_sample_negatives_weighted": [_PG, _vp, _i64, _i32, _i32, _i32, _i64, _i64, _vp, _i64, _vp, _vp, _vp],
    "bess_gather_negative_logq": [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _vp, _vp],
    "bess_sample_bucket_indices": [_PG, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    "bess_lookup_triples": [_vp, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "bess_gather_candidate_lists": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp],
    "bess_known_triple_mask": [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64,
                               _vp, _i64, _i64, _i32, _vp, _i64, _i64, _vp, _i64, _i32, _vp],
    "bess_known_completions": [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp,
                               _vp, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "bess_comm_unique_id": [_c_u8p],
    "bess_comm_init_rank": [_i32, _i32, _c_u8p, ctypes.POINTER(_vp)],
    "bess_comm_init_all": [_i32, _c_i32p, ctypes.POINTER(_vp)],
    "bess_comm_destroy": [_vp],
    "bess_comm_info": [_vp, _c_i32p, _c_i32p, _c_i32p],
    "bess_alltoall": [_vp, _vp, _vp, _i64, _vp],
    "bess_allgather": [_vp, _vp, _vp, _i64, _vp],
    "bess_allreduce_sum_f32": [_vp, _vp, _vp, _i64, _vp],
    "bess_pack_exchange": [_vp, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp],
    "bess_graph_node_counts": [_vp, _c_i32p, _i32],
    "bess_plan_create": [ctypes.POINTER(_vp)],
    "bess_plan_destroy": [_vp],
    "bess_plan_knows": [ctypes.c_char_p],
    "bess_plan_length": [_vp],
    "bess_plan_add_call": [_vp, ctypes.c_char_p, _i32, _c_u8p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_vp),
                           ctypes.POINTER(_i64)],
    "bess_plan_run": [_vp, _vp],
    "bess_direct_update": [ctypes.POINTER(OptDesc), _i32, _i32, _vp, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_i64), _vp, _vp,
                           _vp, _vp, _vp, _vp, _vp, _i64, _f32, _vp],
    "bess_neg_score_shared_bwd_parts_plan": [_MD, _i64, _i64, _c_i32p, _c_i32p],
    "bess_neg_score_shared_bwd_parts": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp],
    "bess_query_triple_bwd_parts": [_MD, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _i32, _i64, _vp,
                                    _vp, _vp, _vp, _vp, _vp],
    "bess_pertriple_tail_supported": [_MD, _i64],
    "bess_pertriple_tail": [_MD, _LD, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _i64, _i64, _vp,
                            _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    "bess_regularize_triples": [_MD, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _f32, _f32, _f32, _i32, _vp, _vp, _vp,
                                _vp, _vp, _vp, _f32, _vp, _vp],
    "bess_query_triple_fwd_jobs": [_MD, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i32, ctypes.POINTER(_vp),
                                   ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_i64), _vp],
    "bess_neg_score_shared_fwd_loss": [_MD, _vp, _i64, _vp, _vp, _i64, _vp, _i64, ctypes.POINTER(KillDesc), _LD, _vp, _vp, _i64,
                                       _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp],
}
COMM_ID_BYTES = 128
AFFINE_COUNT_CHUNK_BYTES = 32 << 20  # BESS_AFFINE_COUNT_CHUNK_BYTES
TICKET_INTS = 544  # BESS_TICKET_INTS
ECOMM_BASE = 10000

_lib: Optional[ctypes.CDLL] = None

# Optional per-launch timing with HIP events recorded on the stream the call is issued to (bench.py's roofline leg,
# profiles/): the log holds (entry point, raw stream, start event, end event) in issue order.
_timing: Optional[list] = None
_timed_names: frozenset = frozenset()

# Entry points that are timed under the name of the call they are a variant of.
TIMING_LABELS = {
    "bess_neg_score_pertriple_fwd_dq_masked": "bess_neg_score_pertriple_fwd_dq",
    "bess_neg_score_shared_fwd_ws": "bess_neg_score_shared_fwd",
    "bess_neg_score_shared_fwd_masked": "bess_neg_score_shared_fwd",
    "bess_neg_score_shared_fwd_pruned": "bess_neg_score_shared_fwd",
    "bess_neg_score_shared_bwd_ws": "bess_neg_score_shared_bwd",
    "bess_neg_score_shared_bwd_parts": "bess_neg_score_shared_bwd",
    "bess_sparse_sgd_lists_axpy": "bess_sparse_sgd_lists",
    "bess_coalesced_update_axpy": "bess_coalesced_update",
    "bess_topk_update_flagged": "bess_topk_update",
    "bess_topk_update_excl": "bess_topk_update",
    "bess_topk_update_flagged_excl": "bess_topk_update",
}


class _Recording(threading.local):
    plan: Optional["Plan"] = None  # the plan the calling host thread is recording (`record_plan`), if any


_recording = _Recording()


def start_kernel_timing(names: Sequence[str]) -> None:
    """Record a HIP event pair around every call whose label is named: an entry point of `TIMING_LABELS` has the
    label given there, every other its own name."""
    global _timing, _timed_names
    _timing, _timed_names = [], frozenset(names)


def kernel_timing_log() -> list:
    """[(entry point, raw stream, start event, end event)] of the timed calls so far, in issue order."""
    return list(_timing or [])


def stop_kernel_timing() -> dict:
    """{label: [milliseconds per launch]} since start_kernel_timing()."""
    global _timing
    rec, _timing = _timing or [], None
    torch.cuda.synchronize()
    out: dict = {}
    for name, _, a, b in rec:
        out.setdefault(TIMING_LABELS.get(name, name), []).append(a.elapsed_time(b))
    return out


def library_path() -> pathlib.Path:
    """In-tree location of the shared library (built by `__graft_entry__.build`)."""
    return pathlib.Path(__file__).parent.absolute() / LIB_NAME


def load() -> ctypes.CDLL:
    """dlopen the HIP library; ImportError if it is missing or ABI-incompatible.

    Same role and failure mode as the reference's `load_custom_ops_so`
    (reference `besskge/__init__.py:10-37`).
    """
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not path.exists():
        raise ImportError(
            f"Cannot find the HIP extension library {LIB_NAME} - tried {[str(path)]}."
            " Build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (or `make -C bess-kge_amd/csrc`)."
        )
    lib = ctypes.CDLL(str(path))
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"{path} does not export {name}") from e
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int64 if name in _RETURNS_I64 else ctypes.c_int
    if lib.bess_version() != ABI_VERSION:
        raise ImportError(
            f"{path}: ABI version {lib.bess_version()} != expected {ABI_VERSION}"
        )
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        buf = ctypes.create_string_buffer(512)
        load().bess_last_error(buf, 512)
        kind = "invalid argument" if rc < 0 else (f"ncclResult {rc - ECOMM_BASE}" if rc >= ECOMM_BASE else f"hipError {rc}")
        raise RuntimeError(f"besskge native call {what} failed ({kind}): {buf.value.decode()}")


# --------------------------------------------------------------------------- #
# tensor checks
def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:
        return F16
    raise TypeError(f"embedding tables must be float32 or float16, got {t.dtype}")


def _dev(t: torch.Tensor, name: str) -> torch.device:
    if not t.is_cuda:
        raise RuntimeError(
            f"besskge: `{name}` is on {t.device}; the BESS hot path runs on"
            " HIP devices only (there is no CPU fallback)"
        )
    return t.device


def _same_device(ts: Sequence[Tuple[str, Optional[torch.Tensor]]]) -> torch.device:
    dev = None
    for name, t in ts:
        if t is None:
            continue
        d = _dev(t, name)
        if dev is None:
            dev = d
        elif d != dev:
            raise RuntimeError(f"besskge: `{name}` is on {d}, expected {dev}")
    assert dev is not None
    return dev


def _rows(base: torch.Tensor, name: str, width: int) -> None:
    if base.dim() != 2 or base.shape[1] != width or not base.is_contiguous():
        raise ValueError(
            f"`{name}` must be a contiguous [rows, {width}] tensor, got"
            f" shape {tuple(base.shape)} stride {base.stride()}"
        )


def _idx(idx: Optional[torch.Tensor], name: str, n: Optional[int] = None) -> int:
    if idx is None:
        return 0
    if idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous():
        raise ValueError(
            f"`{name}` must be a contiguous 1-D int32 tensor, got {idx.dtype} {tuple(idx.shape)}"
        )
    if n is not None and idx.numel() != n:
        raise ValueError(f"`{name}` has {idx.numel()} entries, expected {n}")
    return idx.data_ptr()


def _f32(t: torch.Tensor, name: str) -> None:
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"`{name}` must be contiguous float32, got {t.dtype}")


def _f32s(*named: Tuple[str, torch.Tensor]) -> None:
    for name, t in named:
        _f32(t, name)


def _ptr(t: Optional[torch.Tensor]) -> int:
    """Data pointer of `t`; 0 (NULL) for None."""
    return 0 if t is None else t.data_ptr()


def _mat(t: Optional[torch.Tensor], dtype: Any, msg: str, rows: Optional[Tuple[int, ...]] = None,
         cols: Optional[int] = None, who: Optional[str] = None) -> Tuple[int, int, int]:
    """(pointer, rows, columns) of a contiguous 2-D matrix of `dtype` (one, or a tuple of them) - the mask, id, flag
    and map operands; (0, 0, 0) for None.  `rows` / `cols`: the row counts / the column count it may have.  Anything
    else is a ValueError with the caller's text `msg`, behind "`who`: " if given (joined on this branch only)."""
    if t is None:
        return 0, 0, 0
    if (t.dtype not in dtype if type(dtype) is tuple else t.dtype != dtype) or t.dim() != 2 or not t.is_contiguous() \
            or (rows is not None and t.shape[0] not in rows) or (cols is not None and t.shape[1] != cols):
        raise ValueError(msg if who is None else f"{who}: {msg}")
    return t.data_ptr(), int(t.shape[0]), int(t.shape[1])


_KILL_MASK = "negative_mask must be a contiguous 2-D bool tensor"


def _carve_offsets(lengths: Sequence[int]) -> List[int]:
    """Offsets, in elements of 4 bytes, of pieces of the given lengths laid out one after the other with every piece
    on a 16-byte boundary; the last entry is the total."""
    offs, at = [0], 0
    for n in lengths:
        at += (n + 3) // 4 * 4
        offs.append(at)
    return offs


def _carve_f32(dev: torch.device, *lengths: int) -> List[torch.Tensor]:
    """ONE allocation for several small float32 vectors (`_carve_offsets`): a step makes a handful of them per call,
    and every torch.empty is host time.  Recorded graphs and plans hold addresses inside these buffers: the layout
    is part of what a wrapper does."""
    offs = _carve_offsets(lengths)
    buf = torch.empty((offs[-1],), dtype=torch.float32, device=dev)
    return [buf[o: o + n] for o, n in zip(offs, lengths)]


def _row_count(base: torch.Tensor, idx: Optional[torch.Tensor]) -> int:
    return int(idx.numel()) if idx is not None else int(base.shape[0])


def _stream(dev: torch.device) -> int:
    """Raw handle of PyTorch's current HIP stream on `dev` (no Stream object is built: this runs per launch)."""
    return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())


_NO_SWITCH = contextlib.nullcontext()


def _on(dev: torch.device) -> Any:
    """`torch.cuda.device(dev)` only when `dev` is not the current device already (the usual case: one
    process per GPU) - the context manager costs more host time than the launch it wraps."""
    if dev.index is None or torch.cuda.current_device() == dev.index:
        return _NO_SWITCH
    return torch.cuda.device(dev)


def _launch(name: str, dev: torch.device, *args: Any) -> None:
    """Call entry point `name` with `args` and PyTorch's current stream of `dev`: the one path of every call that puts
    work on a stream.  The call is bracketed with HIP events while its label is timed, and noted in the calling
    thread's plan while that thread records one (`record_plan`)."""
    if dev.index is not None and torch.cuda.current_device() != dev.index:
        with torch.cuda.device(dev):  # (rare: see _on)
            return _launch(name, dev, *args)
    stream = _stream(dev)
    log = _timing
    if log is None or TIMING_LABELS.get(name, name) not in _timed_names:
        rc = getattr(load(), name)(*args, stream)
    else:
        s = torch.cuda.current_stream(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        rc = getattr(load(), name)(*args, stream)
        b.record(s)
        log.append((name, stream, a, b))
    if rc == 0 and _recording.plan is not None:
        _recording.plan._add(name, args)
    _check(rc, name)


class RowSource:
    """`rows[i] = base[idx[i]]` (idx None: identity).  `base` is a contiguous
    [*, W] table-dtype tensor: a shard, a receive buffer or plain embeddings."""

    __slots__ = ("base", "idx")

    def __init__(self, base: torch.Tensor, idx: Optional[torch.Tensor] = None) -> None:
        self.base = base
        self.idx = idx

    def __len__(self) -> int:
        return _row_count(self.base, self.idx)


def copy_desc(d: ModelDesc) -> ModelDesc:
    c = ModelDesc()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(d), ctypes.sizeof(ModelDesc))
    return c


def with_row_count(d: ModelDesc, base: torch.Tensor) -> ModelDesc:
    """TransE / RotatE / DistMult / ComplEx: a copy of `d` with desc.reserved[1] = the rows of `base` (the table the
    negative ids index), which lets bess_neg_score_pertriple_fwd score tables whose rows recur in row order
    (bess_neg_pertriple_sweep).  Other scorers use reserved[1] for their own settings: `d` as it is."""
    if d.scorer > COMPLEX:
        return d
    c = copy_desc(d)
    rows = int(base.shape[0])
    c.reserved[1] = rows if rows < (1 << 31) else 0
    return c


def pertriple_sweep(d: ModelDesc, n_query: int, n_neg: int) -> bool:
    """Whether bess_neg_score_pertriple_fwd takes the row-ordered kernel for these sizes (host arithmetic)."""
    out = ctypes.c_int32(0)
    _check(load().bess_neg_pertriple_sweep(ctypes.byref(d), n_query, n_neg, ctypes.byref(out)), "bess_neg_pertriple_sweep")
    return bool(out.value)


def make_desc(scorer: int, norm_p: int, table: torch.Tensor, rel_width: int) -> ModelDesc:
    d = ModelDesc()
    d.scorer = scorer
    d.norm_p = norm_p
    d.dtype = _dtype_code(table)
    d.width = int(table.shape[-1])
    d.rel_width = rel_width
    return d


# --------------------------------------------------------------------------- #
# wrappers (one per C entry point)
def gather_rows(table: torch.Tensor, idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    dev = _same_device([("table", table), ("idx", idx), ("out", out)])
    W = int(table.shape[1])
    _rows(table, "table", W)
    n = idx.numel()
    ip = _idx(idx, "idx")
    if out is None:
        out = torch.empty((n, W), dtype=table.dtype, device=dev)
    else:
        _rows(out, "out", W)
        if out.shape[0] != n or out.dtype != table.dtype:
            raise ValueError("gather_rows: `out` does not match idx / table dtype")
    _launch("bess_gather_rows", dev, _dtype_code(table), W, table.data_ptr(), ip, n, out.data_ptr())
    return out


def _triple_operands(d: ModelDesc, head: RowSource, tail: RowSource, rel_table: torch.Tensor, rel_idx: torch.Tensor):
    dev = _same_device(
        [("head", head.base), ("head_idx", head.idx), ("tail", tail.base), ("tail_idx", tail.idx),
         ("relation_embedding", rel_table), ("relation", rel_idx)]
    )
    _rows(head.base, "head rows", d.width)
    _rows(tail.base, "tail rows", d.width)
    _rows(rel_table, "relation_embedding", d.rel_width)
    for t, nm in ((head.base, "head rows"), (tail.base, "tail rows"), (rel_table, "relation_embedding")):
        if _dtype_code(t) != d.dtype:
            raise TypeError(f"`{nm}` dtype {t.dtype} does not match the model descriptor")
    n = len(head)
    if len(tail) != n:
        raise ValueError(f"{n} head rows but {len(tail)} tail rows")
    _idx(rel_idx, "relation", n)
    return dev, n


def score_triple_fwd(d: ModelDesc, head: RowSource, tail: RowSource, rel_table: torch.Tensor,
                     rel_idx: torch.Tensor) -> torch.Tensor:
    dev, n = _triple_operands(d, head, tail, rel_table, rel_idx)
    out = torch.empty((n,), dtype=torch.float32, device=dev)
    _launch("bess_score_triple_fwd", dev, ctypes.byref(d), head.base.data_ptr(), _idx(head.idx, "head_idx"),
            tail.base.data_ptr(), _idx(tail.idx, "tail_idx"), rel_table.data_ptr(), rel_idx.data_ptr(), n,
            out.data_ptr())
    return out


def score_triple_bwd(d: ModelDesc, head: RowSource, tail: RowSource, rel_table: torch.Tensor,
                     rel_idx: torch.Tensor, d_out: torch.Tensor, d_rel_table: torch.Tensor
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (d_head [n, W], d_tail [n, W]); accumulates into d_rel_table."""
    dev, n = _triple_operands(d, head, tail, rel_table, rel_idx)
    _same_device([("d_out", d_out), ("d_rel_table", d_rel_table), ("x", head.base)])
    _f32(d_out, "d_out")
    _f32(d_rel_table, "d_rel_table")
    if d_out.numel() != n or tuple(d_rel_table.shape) != tuple(rel_table.shape):
        raise ValueError("score_triple_bwd: gradient shapes do not match")
    dh = torch.empty((n, d.width), dtype=torch.float32, device=dev)
    dt = torch.empty((n, d.width), dtype=torch.float32, device=dev)
    _launch("bess_score_triple_bwd", dev, ctypes.byref(d), head.base.data_ptr(), _idx(head.idx, "head_idx"),
            tail.base.data_ptr(), _idx(tail.idx, "tail_idx"), rel_table.data_ptr(), rel_idx.data_ptr(), n,
            d_out.data_ptr(), dh.data_ptr(), dt.data_ptr(), d_rel_table.data_ptr())
    return dh, dt


def _job_arrays(jobs: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor], int]], who: str):
    """ctypes arrays (dst, src, value, words) of copy / fill jobs over 4-byte elements (`step_prologue`)."""
    nj = len(jobs)
    if nj > MAX_WORD_JOBS:
        raise ValueError(f"{who}: too many jobs")
    dst, src = (_vp * max(1, nj))(), (_vp * max(1, nj))()
    val, words = (ctypes.c_uint32 * max(1, nj))(), (_i64 * max(1, nj))()
    for i, (d_, s_, v_) in enumerate(jobs):
        if d_.element_size() != 4 or not d_.is_contiguous():
            raise ValueError(f"{who}: job targets must be contiguous tensors of 4-byte elements")
        if s_ is not None and (s_.element_size() != 4 or not s_.is_contiguous() or s_.numel() != d_.numel()):
            raise ValueError(f"{who}: a job's source must match its target")
        dst[i], src[i], val[i], words[i] = d_.data_ptr(), _ptr(s_), int(v_), d_.numel()
    return dst, src, val, words


def query_triple_fwd(d: ModelDesc, side: int, head: RowSource, tail: RowSource, rel_table: torch.Tensor,
                     rel_idx: torch.Tensor, jobs: Optional[Sequence[Tuple[torch.Tensor, Optional[torch.Tensor], int]]] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(query [n, W], positive score [n]) in one launch.  `jobs`: copy / fill jobs as `step_prologue` takes them, run
    by spare workgroups of the same launch (`bess_query_triple_fwd_jobs`)."""
    dev, n = _triple_operands(d, head, tail, rel_table, rel_idx)
    q = torch.empty((n, d.width), dtype=torch.float32, device=dev)
    out = torch.empty((n,), dtype=torch.float32, device=dev)
    if jobs:
        _same_device([("query rows", head.base)] + [("job dst", j[0]) for j in jobs] + [("job src", j[1]) for j in jobs])
        dst, src, val, words = _job_arrays(jobs, "query_triple_fwd")
        _launch("bess_query_triple_fwd_jobs", dev, ctypes.byref(d), side, head.base.data_ptr(),
                _idx(head.idx, "head_idx"), tail.base.data_ptr(), _idx(tail.idx, "tail_idx"), rel_table.data_ptr(),
                rel_idx.data_ptr(), n, q.data_ptr(), out.data_ptr(), len(jobs), dst, src, val, words)
        return q, out
    _launch("bess_query_triple_fwd", dev, ctypes.byref(d), side, head.base.data_ptr(), _idx(head.idx, "head_idx"),
            tail.base.data_ptr(), _idx(tail.idx, "tail_idx"), rel_table.data_ptr(), rel_idx.data_ptr(), n, q.data_ptr(),
            out.data_ptr())
    return q, out


def query_triple_bwd(d: ModelDesc, side: int, head: RowSource, tail: RowSource, rel_table: torch.Tensor,
                     rel_idx: torch.Tensor, d_out: torch.Tensor, d_query: torch.Tensor, d_rel_table: torch.Tensor
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d_head [n, W], d_tail [n, W]) of positive score and query together; accumulates into d_rel_table."""
    dev, n = _triple_operands(d, head, tail, rel_table, rel_idx)
    _same_device([("d_out", d_out), ("d_query", d_query), ("d_rel_table", d_rel_table), ("x", head.base)])
    _f32s(("d_out", d_out), ("d_query", d_query), ("d_rel_table", d_rel_table))
    if d_out.numel() != n or tuple(d_query.shape) != (n, d.width) or tuple(d_rel_table.shape) != tuple(rel_table.shape):
        raise ValueError("query_triple_bwd: gradient shapes do not match")
    dh = torch.empty((n, d.width), dtype=torch.float32, device=dev)
    dt = torch.empty((n, d.width), dtype=torch.float32, device=dev)
    _launch("bess_query_triple_bwd", dev, ctypes.byref(d), side, head.base.data_ptr(), _idx(head.idx, "head_idx"),
            tail.base.data_ptr(), _idx(tail.idx, "tail_idx"), rel_table.data_ptr(), rel_idx.data_ptr(), n,
            d_out.data_ptr(), d_query.data_ptr(), dh.data_ptr(), dt.data_ptr(), d_rel_table.data_ptr())
    return dh, dt


def _query_operands(d: ModelDesc, ent: RowSource, rel_table: torch.Tensor, rel_idx: torch.Tensor):
    dev = _same_device([("entity rows", ent.base), ("entity idx", ent.idx),
                        ("relation_embedding", rel_table), ("relation", rel_idx)])
    _rows(ent.base, "entity rows", d.width)
    _rows(rel_table, "relation_embedding", d.rel_width)
    if _dtype_code(ent.base) != d.dtype or _dtype_code(rel_table) != d.dtype:
        raise TypeError("query: operand dtype does not match the model descriptor")
    n = len(ent)
    _idx(rel_idx, "relation", n)
    return dev, n


def query_fwd(d: ModelDesc, side: int, ent: RowSource, rel_table: torch.Tensor, rel_idx: torch.Tensor) -> torch.Tensor:
    dev, n = _query_operands(d, ent, rel_table, rel_idx)
    q = torch.empty((n, query_width(d)), dtype=torch.float32, device=dev)
    _launch("bess_query_fwd", dev, ctypes.byref(d), side, ent.base.data_ptr(), _idx(ent.idx, "entity idx"),
            rel_table.data_ptr(), rel_idx.data_ptr(), n, q.data_ptr())
    return q


def query_bwd(d: ModelDesc, side: int, ent: RowSource, rel_table: torch.Tensor, rel_idx: torch.Tensor,
              d_query: torch.Tensor, d_rel_table: torch.Tensor) -> torch.Tensor:
    """Returns d_ent [n, W]; accumulates into d_rel_table."""
    dev, n = _query_operands(d, ent, rel_table, rel_idx)
    _same_device([("d_query", d_query), ("d_rel_table", d_rel_table), ("x", ent.base)])
    _f32(d_query, "d_query")
    _f32(d_rel_table, "d_rel_table")
    if tuple(d_query.shape) != (n, query_width(d)) or tuple(d_rel_table.shape) != tuple(rel_table.shape):
        raise ValueError("query_bwd: gradient shapes do not match")
    dx = torch.empty((n, d.width), dtype=torch.float32, device=dev)
    _launch("bess_query_bwd", dev, ctypes.byref(d), side, ent.base.data_ptr(), _idx(ent.idx, "entity idx"),
            rel_table.data_ptr(), rel_idx.data_ptr(), n, d_query.data_ptr(), dx.data_ptr(), d_rel_table.data_ptr())
    return dx


def query_width(d: ModelDesc) -> int:
    """Scalars per row of the query matrix the negative-scoring kernels take."""
    if d.scorer == AFFINE:  # [U | V | R]: one d-wide vector per entity part, plus the offset
        n_part = int(d.reserved[0])
        return (n_part + 1) * (d.width // n_part)
    if d.scorer == BOXE:  # [S | C | H] for each of the two candidate parts
        return 3 * d.width
    return int(d.width)


def _neg_operands(d: ModelDesc, query: torch.Tensor, neg: RowSource, n_idx: int):
    dev = _same_device([("query", query), ("negative rows", neg.base), ("negative idx", neg.idx)])
    _f32(query, "query")
    if query.dim() != 2 or query.shape[1] != query_width(d):
        raise ValueError(f"`query` must be [n_query, {query_width(d)}], got {tuple(query.shape)}")
    _rows(neg.base, "negative rows", d.width)
    if _dtype_code(neg.base) != d.dtype:
        raise TypeError("negative rows dtype does not match the model descriptor")
    if len(neg) != n_idx:
        raise ValueError(f"expected {n_idx} negative rows, got {len(neg)}")
    return dev


def _neg_idx_ptr(neg: RowSource, dev: torch.device) -> Tuple[int, Optional[torch.Tensor]]:
    """The per-triple kernel needs an explicit index array."""
    if neg.idx is not None:
        return _idx(neg.idx, "negative idx"), None
    ar = torch.arange(neg.base.shape[0], dtype=torch.int32, device=dev)
    return ar.data_ptr(), ar


def neg_score_pertriple_fwd(d: ModelDesc, query: torch.Tensor, neg: RowSource, n_neg: int,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    nq = int(query.shape[0])
    dev = _neg_operands(d, query, neg, nq * n_neg)
    if out is None:
        out = torch.empty((nq, n_neg), dtype=torch.float32, device=dev)
    _f32(out, "out")
    if tuple(out.shape) != (nq, n_neg):
        raise ValueError("neg_score_pertriple_fwd: bad `out` shape")
    ip, keep = _neg_idx_ptr(neg, dev)  # (`keep`: the index array lives to the end of the call)
    d = with_row_count(d, neg.base)
    _launch("bess_neg_score_pertriple_fwd", dev, ctypes.byref(d), query.data_ptr(), nq, neg.base.data_ptr(), ip, n_neg,
            out.data_ptr(), n_neg)
    return out


def neg_score_pertriple_fwd_dq(d: ModelDesc, l: LossDesc, query: torch.Tensor, neg: RowSource, n_neg: int,
                               pos: Optional[torch.Tensor], weight: torch.Tensor, mask: Optional[torch.Tensor] = None,
                               defer: bool = False) -> Tuple[torch.Tensor, Any]:
    """Fused training forward: (scores [nq, n_neg], d loss / d query [nq, W]) in one pass over
    the negative rows.  Only valid when the loss is taken over exactly these scores; `mask` (bool
    [1 | nq, cols <= n_neg], False = masked out, over the last `cols` columns) is applied inside the pass.
    `defer`: the second item is (state_ml, state_acc) - the work items' partials, which `pertriple_tail`
    turns into d loss / d query where it uses it."""
    nq = int(query.shape[0])
    dev = _neg_operands(d, query, neg, nq * n_neg)
    _same_device([("pos", pos), ("weight", weight), ("query", query)])
    _f32(weight, "weight")
    if weight.numel() not in (1, nq):
        raise ValueError("triple weights must have 1 or n_query entries")
    if pos is not None:
        _f32(pos, "pos")
        if pos.numel() != nq:
            raise ValueError("`pos` must have n_query entries")
    out, dq, st_ml, st_acc = _partials_buffers(d, nq, n_neg, dev, want_dq=not defer)
    ip, keep = _neg_idx_ptr(neg, dev)
    if mask is not None:
        _same_device([("mask", mask), ("query", query)])
    mp, mrows, mcols = _mat(mask, (torch.bool, torch.uint8),
                            "neg_score_pertriple_fwd_dq: `mask` must be a contiguous 2-D bool / uint8 tensor")
    _launch("bess_neg_score_pertriple_fwd_dq_masked", dev, ctypes.byref(d), ctypes.byref(l), query.data_ptr(), nq,
            neg.base.data_ptr(), ip, n_neg, _ptr(pos), weight.data_ptr(), weight.numel(), mp, mrows, mcols,
            out.data_ptr(), n_neg, _ptr(dq), st_ml.data_ptr(), st_acc.data_ptr())
    return out, ((st_ml, st_acc) if defer else dq)


def _partials_buffers(d: ModelDesc, nq: int, n_neg: int, dev: torch.device, want_dq: bool = False
                      ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """(scores [nq, n_neg], d_query [nq, W] | None, state_ml [nq, items, 2], state_acc [nq, items, W]) of the fused
    per-triple forwards, allocated in this order; `items`: the work items the library splits a query's negatives into."""
    items = ctypes.c_int32(0)
    _check(load().bess_neg_pertriple_items(ctypes.byref(d), nq, n_neg, ctypes.byref(items)), "bess_neg_pertriple_items")
    out = torch.empty((nq, n_neg), dtype=torch.float32, device=dev)
    dq = torch.empty((nq, d.width), dtype=torch.float32, device=dev) if want_dq else None
    st_ml = torch.empty((nq, items.value, 2), dtype=torch.float32, device=dev)
    st_acc = torch.empty((nq, items.value, d.width), dtype=torch.float32, device=dev)
    return out, dq, st_ml, st_acc


def pertriple_tail_supported(d: ModelDesc, n_neg: int) -> bool:
    return bool(load().bess_pertriple_tail_supported(ctypes.byref(d), int(n_neg)))


def pertriple_tail(d: ModelDesc, l: LossDesc, side: int, head: RowSource, tail: RowSource, rel_table: torch.Tensor,
                   rel_idx: torch.Tensor, partials: Tuple[torch.Tensor, torch.Tensor], pos: torch.Tensor, neg: torch.Tensor,
                   weight: torch.Tensor, d_rel_table: torch.Tensor, want_d_query: bool = False) -> Tuple[Any, ...]:
    """The per-triple remainder of a training step whose negatives went through the fused forward with `defer=True`
    (`bess_pertriple_tail`, one launch): returns (loss [], d_pos [n], d_neg [n, n_neg], d_head [n, W], d_tail [n, W])
    - and d loss / d query [n, W] as a sixth item with `want_d_query`; relation gradients are added into
    `d_rel_table`."""
    dev, n = _triple_operands(d, head, tail, rel_table, rel_idx)
    st_ml, st_acc = partials
    _same_device([("partials", st_ml), ("partials", st_acc), ("positive_score", pos), ("negative_score", neg),
                  ("triple_weight", weight), ("d_rel_table", d_rel_table), ("x", head.base)])
    _f32s(("partials", st_ml), ("partials", st_acc), ("positive_score", pos), ("negative_score", neg),
          ("triple_weight", weight), ("d_rel_table", d_rel_table))
    N = int(neg.shape[1])
    items = int(st_ml.shape[1])
    if tuple(st_ml.shape) != (n, items, 2) or tuple(st_acc.shape) != (n, items, d.width) or pos.numel() != n \
            or neg.shape[0] != n or weight.numel() not in (1, n) or tuple(d_rel_table.shape) != tuple(rel_table.shape):
        raise ValueError("pertriple_tail: shapes do not match")
    row_loss, dp, loss = _carve_f32(dev, n, n, 1)
    dn = torch.empty((n, N), dtype=torch.float32, device=dev)
    rows = torch.empty((3 if want_d_query else 2, n, d.width), dtype=torch.float32, device=dev)
    counter = _counters(dev, 1)
    _launch("bess_pertriple_tail", dev, ctypes.byref(d), ctypes.byref(l), side, head.base.data_ptr(),
            _idx(head.idx, "head_idx"), tail.base.data_ptr(), _idx(tail.idx, "tail_idx"), rel_table.data_ptr(),
            rel_idx.data_ptr(), n, st_ml.data_ptr(), st_acc.data_ptr(), items, pos.data_ptr(), neg.data_ptr(), N,
            int(neg.stride(0)), weight.data_ptr(), weight.numel(), row_loss.data_ptr(), loss.data_ptr(), dp.data_ptr(),
            dn.data_ptr(), N, rows[2].data_ptr() if want_d_query else 0, rows[0].data_ptr(), rows[1].data_ptr(),
            d_rel_table.data_ptr(), counter.data_ptr())
    res = (loss.reshape(()), dp, dn, rows[0], rows[1])
    return res + (rows[2],) if want_d_query else res


REG_ENTITY_MODULUS = 1  # BESS_REG_ENTITY_MODULUS
REG_RELATION_MODULUS = 2  # BESS_REG_RELATION_MODULUS


def regularize_triples(head: RowSource, tail: RowSource, rel_table: Optional[torch.Tensor],
                       rel_idx: Optional[torch.Tensor], weight: torch.Tensor, p: float, entity_coef: float,
                       relation_coef: float, loss_scale: float = 1.0, flags: int = 0,
                       d_head: Optional[torch.Tensor] = None, d_tail: Optional[torch.Tensor] = None,
                       d_rel_table: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None,
                       loss_factor: float = 1.0) -> torch.Tensor:
    """Lp / N3 penalty on the rows of the triples (`bess_regularize_triples`, one launch): returns the penalty [] f32;
    its gradient is ADDED into `d_head`, `d_tail` [n, W] f32 and (atomically) `d_rel_table` - both None: the value
    only - and `loss_factor` times the penalty into the scalar `loss`, if given.  `rel_table`, `rel_idx` and
    `d_rel_table` may be None with `relation_coef == 0`."""
    dev = _same_device([("head", head.base), ("head_idx", head.idx), ("tail", tail.base), ("tail_idx", tail.idx),
                        ("relation_embedding", rel_table), ("relation", rel_idx), ("triple_weight", weight),
                        ("d_head", d_head), ("d_tail", d_tail), ("d_rel_table", d_rel_table), ("loss", loss)])
    W = int(head.base.shape[-1])
    _rows(head.base, "head rows", W)
    _rows(tail.base, "tail rows", W)
    if tail.base.dtype != head.base.dtype:
        raise TypeError("regularize_triples: head and tail rows differ in dtype")
    n = len(head)
    if len(tail) != n:
        raise ValueError(f"{n} head rows but {len(tail)} tail rows")
    d = ModelDesc()
    d.dtype, d.width, d.rel_width = _dtype_code(head.base), W, W
    if rel_table is not None:
        d.rel_width = int(rel_table.shape[-1])
        _rows(rel_table, "relation_embedding", d.rel_width)
        if rel_table.dtype != head.base.dtype:
            raise TypeError("regularize_triples: relation and entity rows differ in dtype")
        if rel_idx is None:
            raise ValueError("regularize_triples: relation rows without `rel_idx`")
        _idx(rel_idx, "relation", n)
    _f32(weight, "triple_weight")
    for g, nm, shape in ((d_head, "d_head", (n, W)), (d_tail, "d_tail", (n, W)),
                         (d_rel_table, "d_rel_table", tuple(rel_table.shape) if rel_table is not None else None)):
        if g is not None:
            _f32(g, nm)
            if tuple(g.shape) != shape:
                raise ValueError(f"regularize_triples: `{nm}` has shape {tuple(g.shape)}, expected {shape}")
    if loss is not None and (loss.dtype != torch.float32 or loss.numel() != 1):
        raise ValueError("regularize_triples: `loss` must be one float32")
    row_terms, penalty = _carve_f32(dev, n, 1)
    counter = _counters(dev, 1)
    _launch("bess_regularize_triples", dev, ctypes.byref(d), head.base.data_ptr(), _idx(head.idx, "head_idx"),
            tail.base.data_ptr(), _idx(tail.idx, "tail_idx"), _ptr(rel_table), _idx(rel_idx, "relation"), n,
            weight.data_ptr(), weight.numel(), float(p), float(entity_coef), float(relation_coef), float(loss_scale),
            int(flags), _ptr(d_head), _ptr(d_tail), _ptr(d_rel_table), row_terms.data_ptr(), penalty.data_ptr(),
            _ptr(loss), float(loss_factor), counter.data_ptr())
    return penalty.reshape(())


def row_fits_registers(d: ModelDesc) -> bool:
    """Do the per-triple kernels keep a whole row in a 16-lane group's registers (1024 f32 / 2048 f16 scalars at full
    vector width)?  Wider rows are scored in column windows, which the fused training forward cannot use."""
    W = int(d.width)
    vec = 4 if d.dtype == F32 else 8
    if W % vec:
        vec = 2 if (d.dtype == F16 and W % 2 == 0) else 1
    return W <= 256 * vec


def neg_score_pertriple_fwd_partials(d: ModelDesc, l: LossDesc, query: torch.Tensor, neg: RowSource, n_neg: int
                                     ) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """Training forward on a shard that holds only a part of each query's negatives (ScoreMoving): scores
    [nq, n_neg] and the partials (state_ml [nq, items, 2], state_acc [nq, items, W]) that
    `combine_dq_partials` turns into this shard's share of d loss / d query."""
    nq = int(query.shape[0])
    dev = _neg_operands(d, query, neg, nq * n_neg)
    out, _, st_ml, st_acc = _partials_buffers(d, nq, n_neg, dev)
    ip, keep = _neg_idx_ptr(neg, dev)
    _launch("bess_neg_score_pertriple_fwd_partials", dev, ctypes.byref(d), ctypes.byref(l), query.data_ptr(), nq,
            neg.base.data_ptr(), ip, n_neg, out.data_ptr(), n_neg, st_ml.data_ptr(), st_acc.data_ptr())
    return out, (st_ml, st_acc)


def combine_dq_partials(state: Tuple[torch.Tensor, torch.Tensor], norm: torch.Tensor) -> torch.Tensor:
    """d_query [nq, W] of this shard's negatives from its partials and the per-query (m, L / C) of the whole
    softmax, `norm` [nq, 2] f32 (see include/besskge_hip.h)."""
    st_ml, st_acc = state
    nq, items, W = (int(x) for x in st_acc.shape)
    dev = _same_device([("state_ml", st_ml), ("state_acc", st_acc), ("norm", norm)])
    _f32(norm, "norm")
    if tuple(norm.shape) != (nq, 2) or not norm.is_contiguous():
        raise ValueError("combine_dq_partials: `norm` must be a contiguous [n_query, 2] tensor")
    dq = torch.empty((nq, W), dtype=torch.float32, device=dev)
    _launch("bess_combine_dq_partials", dev, st_ml.data_ptr(), st_acc.data_ptr(), nq, items, W, norm.data_ptr(),
            dq.data_ptr())
    return dq


def neg_score_pertriple_bwd(d: ModelDesc, query: torch.Tensor, neg: RowSource, n_neg: int,
                            d_out: torch.Tensor, want_d_neg: bool = True, want_d_query: bool = True,
                            d_neg_rows: Optional[torch.Tensor] = None
                            ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Returns (d_query [nq, W] or None, d_neg [nq*n_neg, W] or None).  `want_d_query=False` (TransE / RotatE /
    DistMult / ComplEx; d_query came out of the fused forward): DistMult / ComplEx then do not read the candidate
    rows at all - their d_neg rows are coefficient x query.  `d_neg_rows` ([rows of neg.base, W] f32; the four
    native scorers): the gradient of reference k is STORED at row neg.idx[k] of it (BESS_FLAG_DNEG_BY_ROW) - only for
    lists that name a row at most once; d_neg is not returned then."""
    nq = int(query.shape[0])
    dev = _neg_operands(d, query, neg, nq * n_neg)
    _same_device([("d_out", d_out), ("query", query)])
    _f32(d_out, "d_out")
    if tuple(d_out.shape) != (nq, n_neg):
        raise ValueError("neg_score_pertriple_bwd: bad `d_out` shape")
    if not want_d_query and (int(d.scorer) > COMPLEX or not want_d_neg):
        raise ValueError("neg_score_pertriple_bwd: want_d_query=False is for the four native scorers, with d_neg")
    dq = torch.empty((nq, query_width(d)), dtype=torch.float32, device=dev) if want_d_query else None
    dn = torch.empty((nq * n_neg, d.width), dtype=torch.float32, device=dev) if want_d_neg else None
    if d_neg_rows is not None:
        if (int(d.scorer) > COMPLEX or not want_d_neg or d_neg_rows.dtype != torch.float32 or not d_neg_rows.is_contiguous()
                or tuple(d_neg_rows.shape) != (int(neg.base.shape[0]), int(d.width)) or d_neg_rows.device != dev):
            raise ValueError("neg_score_pertriple_bwd: `d_neg_rows` must be a contiguous f32 [rows of neg.base, W] "
                             "tensor (native scorers)")
        d = copy_desc(d)
        d.reserved[0] |= FLAG_DNEG_BY_ROW
        dn = d_neg_rows
    ip, keep = _neg_idx_ptr(neg, dev)
    _launch("bess_neg_score_pertriple_bwd", dev, ctypes.byref(d), query.data_ptr(), nq, neg.base.data_ptr(), ip, n_neg,
            d_out.data_ptr(), n_neg, _ptr(dq), _ptr(dn))
    return dq, (None if d_neg_rows is not None else dn)


def normalize_rows(neg: RowSource, n_part: int, normalize: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """Gather + convert to f32 + L2-normalise every part of the rows: (hat [n, W] f32, inv [n, n_part])."""
    dev = _same_device([("rows", neg.base), ("idx", neg.idx)])
    W = int(neg.base.shape[1])
    _rows(neg.base, "rows", W)
    n = len(neg)
    hat = torch.empty((n, W), dtype=torch.float32, device=dev)
    inv = torch.empty((n, n_part), dtype=torch.float32, device=dev)
    _launch("bess_normalize_rows", dev, _dtype_code(neg.base), neg.base.data_ptr(), _idx(neg.idx, "idx"), n, W, n_part,
            int(normalize), hat.data_ptr(), inv.data_ptr())
    return hat, inv


def normalize_rows_bwd(hat: torch.Tensor, inv: torch.Tensor, d_hat: torch.Tensor) -> torch.Tensor:
    dev = _same_device([("hat", hat), ("inv", inv), ("d_hat", d_hat)])
    _f32s(("hat", hat), ("inv", inv), ("d_hat", d_hat))
    if hat.shape != d_hat.shape or inv.shape[0] != hat.shape[0]:
        raise ValueError("normalize_rows_bwd: shape mismatch")
    out = torch.empty_like(hat)
    _launch("bess_normalize_rows_bwd", dev, hat.data_ptr(), inv.data_ptr(), d_hat.data_ptr(), hat.shape[0],
            hat.shape[1], inv.shape[1], out.data_ptr())
    return out


def affine_count_chunk_rows(d: ModelDesc) -> int:
    """Candidate rows per launch of the affine scorers' counting pass (`bess_neg_score_table_fwd_counts`):
    `AFFINE_COUNT_CHUNK_BYTES` of table rows, in whole 64-row tiles, at least one.  Its workspace is the inverse part
    norms of one chunk: at most this many rows x n_part floats, whatever the number of queries."""
    row_bytes = int(d.width) * (4 if d.dtype == F32 else 2)
    return max(64, AFFINE_COUNT_CHUNK_BYTES // row_bytes // 64 * 64)


def _affine_candidates(d: ModelDesc, neg: RowSource) -> Tuple[RowSource, torch.Tensor, torch.Tensor]:
    """The shared kernels of the affine scorers work on dense, normalised f32 candidates."""
    hat, inv = normalize_rows(neg, int(d.reserved[0]), bool(d.reserved[1] & 1))
    return RowSource(hat), hat, inv


def _range_flag(ws: Optional[torch.Tensor], range_flags: Optional[list]) -> None:
    """Note the range flag of a split-fp16 product in `range_flags`: the int32 at the tail of its scratch, non-zero
    after the call when an operand was outside the fp16 range and the fp32 kernels computed the scores instead."""
    if range_flags is not None and ws is not None:
        off = (ws.numel() - 256) // 16 * 16
        range_flags.append(ws[off: off + 4].view(torch.int32))


def _workspace(query: str, d: ModelDesc, nq: int, n_neg: int, dev: torch.device) -> Tuple[Optional[torch.Tensor], int]:
    """(scratch | None, its bytes) that the workspace query `query` asks for: the scratch of the split-fp16
    matrix-core path (0 bytes for the other scorers / small shapes).  From torch's caching allocator, so it is
    stream-ordered and safe under graph capture."""
    ws_bytes = int(getattr(load(), query)(ctypes.byref(d), nq, n_neg))
    return (torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes > 0 else None), ws_bytes


def _kill_desc(kill: Optional[Tuple[int, bool, int, Optional[torch.Tensor]]], query: torch.Tensor) -> Optional[KillDesc]:
    """`kill` = (diag_step, ht, ppp, mask [rows, cols] bool | None) as struct bess_kill_desc; None for None."""
    if kill is None:
        return None
    diag_step, ht, ppp, mask = kill
    kd = KillDesc()
    kd.diag_step, kd.ht, kd.ppp = int(diag_step), int(bool(ht)), int(ppp)
    if mask is not None:
        _same_device([("negative_mask", mask), ("query", query)])
        kd.mask, kd.mask_rows, kd.mask_cols = _mat(mask, torch.bool, _KILL_MASK)
    return kd


def neg_score_shared_fwd(d: ModelDesc, query: torch.Tensor, neg: RowSource, pad_ld: bool = False,
                         kill: Optional[Tuple[int, bool, int, Optional[torch.Tensor]]] = None,
                         range_flags: Optional[list] = None) -> torch.Tensor:
    """Scores [nq, n_neg].  `pad_ld`: rows of the result are 16-B aligned (leading dimension rounded
    up to 4 floats; the result is then a column slice of the buffer) - what `topk_update` streams fastest.
    `kill` = (diag_step, ht, ppp, mask [rows, cols] bool | None): K7 applied with the scores
    (`mask_scores` semantics; in the scoring kernel's epilogue where it has one).  `range_flags`: a list that
    receives the call's range flag when the split-fp16 product ran (`_range_flag`)."""
    nq, n_neg = int(query.shape[0]), len(neg)
    dev = _neg_operands(d, query, neg, n_neg)
    if d.scorer == AFFINE:
        neg, _, _ = _affine_candidates(d, neg)
    ld = (n_neg + 3) // 4 * 4 if pad_ld else n_neg
    out = torch.empty((nq, ld), dtype=torch.float32, device=dev)
    ws, ws_bytes = _workspace("bess_neg_score_shared_workspace", d, nq, n_neg, dev)
    kd = _kill_desc(kill, query)
    if kd is None:
        _launch("bess_neg_score_shared_fwd_ws", dev, ctypes.byref(d), query.data_ptr(), nq, neg.base.data_ptr(),
                _idx(neg.idx, "negative idx"), n_neg, out.data_ptr(), ld, _ptr(ws), ws_bytes)
    else:
        _launch("bess_neg_score_shared_fwd_masked", dev, ctypes.byref(d), query.data_ptr(), nq, neg.base.data_ptr(),
                _idx(neg.idx, "negative idx"), n_neg, out.data_ptr(), ld, ctypes.byref(kd), _ptr(ws), ws_bytes)
    _range_flag(ws, range_flags)
    return out if ld == n_neg else out[:, :n_neg]


def neg_score_shared_fwd_pruned(d: ModelDesc, query: torch.Tensor, neg: RowSource, thr: torch.Tensor,
                                range_flags: Optional[list] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores [nq, n_neg] with 16-B aligned rows, flags [nq, n_blocks] uint8) for the top-k passes: a row's block
    of 64 consecutive candidates is written only when one of its scores is above `thr[row]` (f32 [nq]: the row's
    current k-th best), `flags` marks the blocks that were - the rest of `scores` is uninitialised memory, which
    `topk_update(..., flags=flags)` never reads.  (`bess_neg_score_shared_fwd_pruned`: kernels without a pruning
    epilogue write and flag everything.)  `range_flags`: see `_range_flag`."""
    nq, n_neg = int(query.shape[0]), len(neg)
    dev = _neg_operands(d, query, neg, n_neg)
    _same_device([("query", query), ("thr", thr)])
    _f32(thr, "thr")
    if thr.numel() != nq:
        raise ValueError("neg_score_shared_fwd_pruned: one threshold per query")
    if d.scorer == AFFINE:
        neg, _, _ = _affine_candidates(d, neg)
    ld = (n_neg + 3) // 4 * 4
    out = torch.empty((nq, ld), dtype=torch.float32, device=dev)
    ldf = ((n_neg + 63) // 64 + 3) // 4 * 4
    flags = torch.empty((nq, ldf), dtype=torch.uint8, device=dev)
    ws, ws_bytes = _workspace("bess_neg_score_shared_workspace", d, nq, n_neg, dev)
    _launch("bess_neg_score_shared_fwd_pruned", dev, ctypes.byref(d), query.data_ptr(), nq, neg.base.data_ptr(),
            _idx(neg.idx, "negative idx"), n_neg, out.data_ptr(), ld, thr.data_ptr(), flags.data_ptr(), ldf,
            _ptr(ws), ws_bytes)
    _range_flag(ws, range_flags)
    return (out if ld == n_neg else out[:, :n_neg]), flags


def neg_score_shared_pairs(d: ModelDesc, query: torch.Tensor, neg: RowSource, like_n_query: int,
                           like_n_neg: int) -> torch.Tensor:
    """out[i] = score(query[i], candidate i of `neg`) in the arithmetic of the all-entity pass over a
    (like_n_query x like_n_neg) problem (`bess_neg_score_table_fwd_pairs`: `neg` names rows of the entity table for
    every scorer): what `neg_score_shared_counts` compares against, to the last bit."""
    n = int(query.shape[0])
    if len(neg) != n or neg.idx is None:
        raise ValueError("neg_score_shared_pairs: one indexed candidate per query")
    dev = _neg_operands(d, query, neg, n)
    out = torch.empty((n,), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    ws, ws_bytes = _workspace("bess_neg_score_table_fwd_pairs_workspace", d, int(like_n_query), int(like_n_neg), dev)
    _launch("bess_neg_score_table_fwd_pairs", dev, ctypes.byref(d), query.data_ptr(), neg.base.data_ptr(),
            _idx(neg.idx, "negative idx"), n, int(like_n_query), int(like_n_neg), out.data_ptr(), _ptr(ws), ws_bytes)
    return out


def neg_score_shared_counts(d: ModelDesc, query: torch.Tensor, neg: RowSource, thr: torch.Tensor,
                            excl: torch.Tensor, counts: Optional[torch.Tensor] = None,
                            round_f16: bool = False) -> torch.Tensor:
    """Ranks without the score matrix (`bess_neg_score_table_fwd_counts`; `neg`: rows of the entity table for every
    scorer - the affine family's are normalised as the kernel stages them): adds to `counts` [nq, 2] int32 (made
    and cleared when None) the number of candidates scoring above / exactly `thr[q]` (f32 [nq]: the score of the
    row's true completion), leaving out candidate `excl[q]` (int32 [nq]: its position in `neg`, -1: not among
    them).  `round_f16`: scores are rounded to fp16 before they are compared (the ranking of a half-precision
    model's scores).  Negative counts afterwards: an operand was outside the fp16 range of the matrix-core product - score
    that batch through `neg_score_shared_fwd` instead."""
    nq, n_neg = int(query.shape[0]), len(neg)
    dev = _neg_operands(d, query, neg, n_neg)
    _same_device([("query", query), ("thr", thr), ("excl", excl), ("counts", counts)])
    _f32(thr, "thr")
    if thr.numel() != nq or excl.numel() != nq or excl.dtype != torch.int32:
        raise ValueError("neg_score_shared_counts: one threshold and one excluded position (int32) per query")
    if not thr.is_contiguous() or not excl.is_contiguous():
        raise ValueError("neg_score_shared_counts: thr / excl must be contiguous")
    if counts is None:
        counts = torch.zeros((nq, 2), dtype=torch.int32, device=dev)
    elif tuple(counts.shape) != (nq, 2) or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError("neg_score_shared_counts: counts must be a contiguous [nq, 2] int32 tensor")
    ws, ws_bytes = _workspace("bess_neg_score_table_fwd_counts_workspace", d, nq, n_neg, dev)
    _launch("bess_neg_score_table_fwd_counts", dev, ctypes.byref(d), query.data_ptr(), nq, neg.base.data_ptr(),
            _idx(neg.idx, "negative idx"), n_neg, thr.data_ptr(), excl.data_ptr(), counts.data_ptr(),
            int(bool(round_f16)), _ptr(ws), ws_bytes)
    return counts


def _sized_workspace(query: str, d: ModelDesc, nq: int, n_neg: int, dev: torch.device,
                     workspace_bytes: Optional[int]) -> Tuple[Optional[torch.Tensor], int]:
    """`_workspace`, or a scratch of `workspace_bytes` when the caller sets the size (the tile width of the
    softmax passes follows from it)."""
    if workspace_bytes is None:
        return _workspace(query, d, nq, n_neg, dev)
    ws_bytes = int(workspace_bytes)
    return (torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes > 0 else None), ws_bytes


def neg_score_shared_lse(d: ModelDesc, query: torch.Tensor, neg: RowSource, state_ml: Optional[torch.Tensor] = None,
                         workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """Softmax normaliser over all candidates without the score matrix (`bess_neg_score_shared_fwd_lse`): merges
    the scores of every query against `neg` into `state_ml` [nq, 2] f32 = (running max m, running sum l of
    exp(score - m)) - made empty, (-inf, 0), when None - and returns it; log-sum-exp = m + log(l).  Several calls
    accumulate.  `workspace_bytes`: scratch size instead of the library's default (the score tile of the shapes
    without a fused epilogue is as wide as it allows, whole multiples of 64 columns).  An operand outside the fp16
    range of the matrix-core product (the library answers NaN states): the call is repeated in fp32 arithmetic on
    the state as it was (one host read of a flag, on the matrix-core path only)."""
    nq, n_neg = int(query.shape[0]), len(neg)
    dev = _neg_operands(d, query, neg, n_neg)
    if int(d.scorer) > COMPLEX:
        raise ValueError("neg_score_shared_lse: TransE / RotatE / DistMult / ComplEx only")
    if state_ml is None:
        state_ml = torch.empty((nq, 2), dtype=torch.float32, device=dev)
        state_ml[:, 0] = float("-inf")
        state_ml[:, 1] = 0.0
    else:
        _same_device([("state_ml", state_ml), ("query", query)])
        if tuple(state_ml.shape) != (nq, 2) or state_ml.dtype != torch.float32 or not state_ml.is_contiguous():
            raise ValueError("neg_score_shared_lse: state_ml must be a contiguous [nq, 2] float32 tensor")
    if nq == 0 or n_neg == 0:
        return state_ml

    def run(desc: ModelDesc, ws_bytes: Optional[int]) -> None:
        ws, nbytes = _sized_workspace("bess_neg_score_shared_fwd_lse_workspace", desc, nq, n_neg, dev, ws_bytes)
        _launch("bess_neg_score_shared_fwd_lse", dev, ctypes.byref(desc), query.data_ptr(), nq, neg.base.data_ptr(),
                _idx(neg.idx, "negative idx"), n_neg, state_ml.data_ptr(), _ptr(ws), nbytes)

    # (the matrix-core path is the only one that can answer NaN for finite operands)
    fused = int(load().bess_neg_score_shared_workspace(ctypes.byref(d), nq, n_neg)) > 0
    before = state_ml.clone() if fused else None
    run(d, workspace_bytes)
    if fused and bool(torch.isnan(state_ml).any()) and not bool(torch.isnan(before).any()):
        state_ml.copy_(before)
        exact = copy_desc(d)
        exact.reserved[0] |= FLAG_FP32_MATH
        run(exact, None)
    return state_ml


def neg_score_shared_bwd_softmax(d: ModelDesc, query: torch.Tensor, neg: RowSource, lse: torch.Tensor,
                                 coef: torch.Tensor, d_query: Optional[torch.Tensor] = None,
                                 workspace_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Backward of a softmax over all candidates without the score matrix (`bess_neg_score_shared_bwd_softmax`):
    with P[q, j] = coef[q] * exp(score(q, j) - lse[q]), returns (d_query [nq, W] with sum_j P dscore/dquery ADDED
    to what it held - zeros when None -, d_neg [n_neg, W] = sum_q P dscore/dcandidate in candidate order)."""
    nq, n_neg = int(query.shape[0]), len(neg)
    dev = _neg_operands(d, query, neg, n_neg)
    if int(d.scorer) > COMPLEX:
        raise ValueError("neg_score_shared_bwd_softmax: TransE / RotatE / DistMult / ComplEx only")
    _same_device([("lse", lse), ("coef", coef), ("d_query", d_query), ("query", query)])
    _f32s(("lse", lse), ("coef", coef))
    if lse.numel() != nq or coef.numel() != nq or not lse.is_contiguous() or not coef.is_contiguous():
        raise ValueError("neg_score_shared_bwd_softmax: one contiguous lse and coef per query")
    W = int(d.width)
    if d_query is None:
        d_query = torch.zeros((nq, W), dtype=torch.float32, device=dev)
    elif tuple(d_query.shape) != (nq, W) or d_query.dtype != torch.float32 or not d_query.is_contiguous():
        raise ValueError("neg_score_shared_bwd_softmax: d_query must be a contiguous [nq, W] float32 tensor")
    d_neg = torch.empty((n_neg, W), dtype=torch.float32, device=dev)
    if nq == 0 or n_neg == 0:
        return d_query, d_neg.zero_()
    ws, ws_bytes = _sized_workspace("bess_neg_score_shared_bwd_softmax_workspace", d, nq, n_neg, dev, workspace_bytes)
    _launch("bess_neg_score_shared_bwd_softmax", dev, ctypes.byref(d), query.data_ptr(), nq, neg.base.data_ptr(),
            _idx(neg.idx, "negative idx"), n_neg, lse.data_ptr(), coef.data_ptr(), d_query.data_ptr(),
            d_neg.data_ptr(), _ptr(ws), ws_bytes)
    return d_query, d_neg


def shared_bwd_buffer(d: ModelDesc, nq: int, n_neg: int, device: torch.device) -> Optional[torch.Tensor]:
    """The [nq + n_neg, W] f32 allocation that `neg_score_shared_bwd(..., prezeroed=buf)` takes for d_query and
    d_neg when a caller clears it itself (with the other fills of its step: `step_prologue`); None for scorers
    whose query and candidate rows differ in width."""
    if query_width(d) != d.width or d.scorer == AFFINE:
        return None
    return torch.empty((nq + n_neg, d.width), dtype=torch.float32, device=device)


def shared_bwd_parts_plan(d: ModelDesc, nq: int, n_neg: int) -> Tuple[int, int]:
    """(n_dq_parts, n_dneg_parts) of `neg_score_shared_bwd_parts` for this scorer and shape; (0, 0): no such form."""
    a, b = ctypes.c_int32(0), ctypes.c_int32(0)
    _check(load().bess_neg_score_shared_bwd_parts_plan(ctypes.byref(d), int(nq), int(n_neg), ctypes.byref(a), ctypes.byref(b)),
           "bess_neg_score_shared_bwd_parts_plan")
    return a.value, b.value


def neg_score_shared_bwd_parts(d: ModelDesc, query: torch.Tensor, neg: RowSource, d_out: torch.Tensor
                               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dq_parts [n_dq, nq, W], dneg_parts [n_de, n_neg, W]): the two products of the shared-negative backward as
    partial sums, written with plain stores - no atomics, nothing to clear (`bess_neg_score_shared_bwd_parts`);
    `query_triple_bwd_parts` adds them up where it consumes them."""
    nq, n_neg = int(query.shape[0]), len(neg)
    dev = _neg_operands(d, query, neg, n_neg)
    _same_device([("d_out", d_out), ("query", query)])
    _f32(d_out, "d_out")
    if tuple(d_out.shape) != (nq, n_neg):
        raise ValueError("neg_score_shared_bwd_parts: bad score-gradient shape")
    n_dq, n_de = shared_bwd_parts_plan(d, nq, n_neg)
    if n_dq == 0:
        raise RuntimeError("neg_score_shared_bwd_parts: this scorer / shape has no partial-sum form")
    W = int(d.width)
    buf = torch.empty((n_dq * nq + n_de * n_neg, W), dtype=torch.float32, device=dev)
    dqp, dep = buf[: n_dq * nq].view(n_dq, nq, W), buf[n_dq * nq:].view(n_de, n_neg, W)
    _launch("bess_neg_score_shared_bwd_parts", dev, ctypes.byref(d), query.data_ptr(), nq, neg.base.data_ptr(),
            _idx(neg.idx, "negative idx"), n_neg, d_out.data_ptr(), n_neg, dqp.data_ptr(), dep.data_ptr())
    return dqp, dep


def query_triple_bwd_parts(d: ModelDesc, side: int, head: RowSource, tail: RowSource, rel_table: torch.Tensor,
                           rel_idx: torch.Tensor, d_out: torch.Tensor, dq_parts: torch.Tensor, dneg_parts: torch.Tensor,
                           neg_idx: torch.Tensor, rows_acc: Tuple[torch.Tensor, torch.Tensor, torch.Tensor],
                           d_rel_table: torch.Tensor) -> None:
    """`query_triple_bwd` by row, fed by the partial sums of `neg_score_shared_bwd_parts`: the heads' and tails' gradient
    rows are added into `rows_acc[0]` / `rows_acc[1]` at the triples' row ids, the candidates' summed rows into
    `rows_acc[2]` at theirs.  rows_acc = accumulators over the row
    spaces of (head.base, tail.base, the candidates' table)."""
    dev, n = _triple_operands(d, head, tail, rel_table, rel_idx)
    acc_h, acc_t, acc_n = rows_acc
    _same_device([("d_out", d_out), ("dq_parts", dq_parts), ("dneg_parts", dneg_parts), ("neg_idx", neg_idx),
                  ("d_rel_table", d_rel_table), ("acc_h", acc_h), ("acc_t", acc_t), ("acc_n", acc_n)])
    _f32s(("d_out", d_out), ("dq_parts", dq_parts), ("dneg_parts", dneg_parts), ("d_rel_table", d_rel_table),
          ("acc_h", acc_h), ("acc_t", acc_t), ("acc_n", acc_n))
    W = int(d.width)
    n_neg = int(neg_idx.numel())
    if dq_parts.dim() != 3 or tuple(dq_parts.shape[1:]) != (n, W) or dneg_parts.dim() != 3 \
            or tuple(dneg_parts.shape[1:]) != (n_neg, W) or d_out.numel() != n or head.idx is None or tail.idx is None \
            or tuple(d_rel_table.shape) != tuple(rel_table.shape):
        raise ValueError("query_triple_bwd_parts: shapes do not match")
    if tuple(acc_h.shape) != (int(head.base.shape[0]), W) or tuple(acc_t.shape) != (int(tail.base.shape[0]), W) \
            or acc_n.dim() != 2 or acc_n.shape[1] != W:
        raise ValueError("query_triple_bwd_parts: accumulators must cover the row spaces of the tables")
    _launch("bess_query_triple_bwd_parts", dev, ctypes.byref(d), side, head.base.data_ptr(), _idx(head.idx, "head_idx"),
            tail.base.data_ptr(), _idx(tail.idx, "tail_idx"), rel_table.data_ptr(), rel_idx.data_ptr(), n,
            d_out.data_ptr(), dq_parts.data_ptr(), int(dq_parts.shape[0]), dneg_parts.data_ptr(),
            int(dneg_parts.shape[0]), n_neg, _idx(neg_idx, "neg_idx", n_neg), acc_h.data_ptr(), acc_t.data_ptr(),
            acc_n.data_ptr(), d_rel_table.data_ptr())


def neg_score_shared_bwd(d: ModelDesc, query: torch.Tensor, neg: RowSource, out: torch.Tensor,
                         d_out: torch.Tensor, prezeroed: Optional[torch.Tensor] = None
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (d_query [nq, W], d_neg [n_neg, W]).  `prezeroed`: a `shared_bwd_buffer` the caller has
    already cleared on this stream - the call then writes into it and does not clear anything."""
    nq, n_neg = int(query.shape[0]), len(neg)
    dev = _neg_operands(d, query, neg, n_neg)
    _same_device([("d_out", d_out), ("out", out), ("query", query)])
    _f32(d_out, "d_out")
    _f32(out, "out")
    if tuple(d_out.shape) != (nq, n_neg) or tuple(out.shape) != (nq, n_neg):
        raise ValueError("neg_score_shared_bwd: bad score shapes")
    hat = inv = None
    if d.scorer == AFFINE:
        neg, hat, inv = _affine_candidates(d, neg)
    qw = query_width(d)
    if prezeroed is not None:
        if tuple(prezeroed.shape) != (nq + n_neg, d.width) or prezeroed.dtype != torch.float32 or qw != d.width:
            raise ValueError("neg_score_shared_bwd: `prezeroed` must come from shared_bwd_buffer()")
        dq, dn = prezeroed[:nq], prezeroed[nq:]
        d = copy_desc(d)
        d.reserved[0] |= FLAG_PREZEROED
    elif qw == d.width:  # one allocation: the library then zeroes both partial-sum targets with one memset
        both = torch.empty(((nq + n_neg), qw), dtype=torch.float32, device=dev)
        dq, dn = both[:nq], both[nq:]
    else:
        dq = torch.empty((nq, qw), dtype=torch.float32, device=dev)
        dn = torch.empty((n_neg, d.width), dtype=torch.float32, device=dev)
    ws, ws_bytes = _workspace("bess_neg_score_shared_bwd_workspace", d, nq, n_neg, dev)
    _launch("bess_neg_score_shared_bwd_ws", dev, ctypes.byref(d), query.data_ptr(), nq, neg.base.data_ptr(),
            _idx(neg.idx, "negative idx"), n_neg, out.data_ptr(), n_neg, d_out.data_ptr(), n_neg, dq.data_ptr(),
            dn.data_ptr(), _ptr(ws), ws_bytes)
    if hat is not None and (d.reserved[1] & 1):
        dn = normalize_rows_bwd(hat, inv, dn)
    return dq, dn


def mask_scores(neg: torch.Tensor, diag_step: int, ht: bool, ppp: int, mask: Optional[torch.Tensor]) -> None:
    """In place K7 (see include/besskge_hip.h)."""
    dev = _same_device([("negative_score", neg), ("negative_mask", mask)])
    _f32(neg, "negative_score")
    if neg.dim() != 2:
        raise ValueError("negative_score must be 2-D")
    S, N = int(neg.shape[0]), int(neg.shape[1])
    mp, mrows, mcols = _mat(mask, torch.bool, _KILL_MASK)
    _launch("bess_mask_scores", dev, neg.data_ptr(), S, N, N, diag_step, int(ht), ppp, mp, mrows, mcols)


# (device, raw stream) -> int32 [TICKET_INTS], zero between calls.  Kept apart from `_counters` on purpose: under stream
# capture this cache allocates where `_counters` raises, and it holds 544 ints, not >= 1024 - merging the two would
# change what a recorded graph contains.
_loss_counters: dict = {}


def loss_fwd_bwd(l: LossDesc, pos: torch.Tensor, neg: torch.Tensor, weight: torch.Tensor, want_grad: bool,
                 want_norm: bool = False, logq: Optional[torch.Tensor] = None, ppp: int = 0,
                 lead_logq: float = 0.0) -> Tuple[Any, ...]:
    """Returns (loss [] f32, d_pos [S] | None, d_neg [S, N] | None) - and, with `want_norm`, a fourth item:
    (m, L / C) of every row's softmax, [S, 2] (what `combine_dq_partials` takes; include/besskge_hip.h).

    `logq` (sampled softmax only, `bess_loss_fwd_bwd_logq`): float32 [1 | 2 | S, C <= N] log-proposals of the last C
    columns, subtracted from their scores inside the kernel (`neg` is not modified); the columns in front of them
    take `lead_logq`.  Two rows are the heads' / tails' halves of every block of `ppp` triples (flat "ht")."""
    dev = _same_device([("positive_score", pos), ("negative_score", neg), ("triple_weight", weight),
                        ("negative_logq", logq)])
    _f32s(("positive_score", pos), ("negative_score", neg), ("triple_weight", weight))
    S, N = int(neg.shape[0]), int(neg.shape[1])
    if pos.numel() != S or weight.numel() not in (1, S):
        raise ValueError("loss: shapes of positive_score / triple_weight do not match negative_score")
    if logq is not None:
        _f32(logq, "negative_logq")
        if logq.dim() != 2:
            raise ValueError("negative_logq must be 2-D")
    row_loss = torch.empty((S,), dtype=torch.float32, device=dev)
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    dp = torch.empty((S,), dtype=torch.float32, device=dev) if want_grad else None
    dn = torch.empty((S, N), dtype=torch.float32, device=dev) if want_grad else None
    norm = torch.empty((S, 2), dtype=torch.float32, device=dev) if want_norm else None
    # (one launch: its last workgroup sums the row terms; the counter it needs is zero between calls)
    capturing = _capturing(dev)
    key = (dev, "capture") if capturing else (dev, _stream(dev))
    counter = _loss_counters.get(key)
    if counter is None:
        counter = _loss_counters[key] = torch.zeros((TICKET_INTS,), dtype=torch.int32, device=dev)
        if not capturing and (dev, "capture") not in _loss_counters:
            # the counter of recorded steps exists before any recording starts (a tensor made while a
            # stream is capturing would be cleared by a fill node at every replay: one more dispatch)
            _loss_counters[(dev, "capture")] = torch.zeros((TICKET_INTS,), dtype=torch.int32, device=dev)
    common = (ctypes.byref(l), pos.data_ptr(), neg.data_ptr(), S, N, N, weight.data_ptr(), weight.numel(),
              row_loss.data_ptr(), loss.data_ptr(), _ptr(dp), _ptr(dn), N, _ptr(norm), counter.data_ptr())
    if logq is not None:
        _launch("bess_loss_fwd_bwd_logq", dev, *common, logq.data_ptr(), int(logq.shape[0]), int(logq.shape[1]),
                int(ppp), float(lead_logq))
    else:
        _launch("bess_loss_fwd_bwd_one_launch", dev, *common)
    if want_norm:
        return loss.reshape(()), dp, dn, norm
    return loss.reshape(()), dp, dn


_tail_counters: dict = {}  # (device, raw stream | "capture", slots) -> int32 [slots], zero between calls


def _capturing(dev: torch.device) -> bool:
    """Is PyTorch's current stream of `dev` being captured into a graph?"""
    with _on(dev):
        return torch.cuda.is_current_stream_capturing()


def _counters(dev: torch.device, slots: int) -> torch.Tensor:
    """Zeroed int32 counters that kernels of one stream leave zero again (one array per stream of `dev`; recorded
    steps share one that exists before any recording starts - a tensor made while a stream is capturing would be
    cleared by a fill node at every replay)."""
    slots = max(1024, 1 << (slots - 1).bit_length())  # (>= BESS_TICKET_INTS)
    capturing = _capturing(dev)
    key = (dev, "capture" if capturing else _stream(dev), slots)
    c = _tail_counters.get(key)
    if c is None:
        if capturing:
            raise RuntimeError("besskge: the counters of a recorded step must exist before the recording starts "
                               "(run the step once eagerly first - Runner does)")
        c = _tail_counters[key] = torch.zeros((slots,), dtype=torch.int32, device=dev)
        _tail_counters.setdefault((dev, "capture", slots), torch.zeros((slots,), dtype=torch.int32, device=dev))
    return c


def neg_score_shared_fwd_loss(d: ModelDesc, l: LossDesc, query: torch.Tensor, neg: RowSource, pos: torch.Tensor,
                              weight: torch.Tensor, kill: Optional[Tuple[int, bool, int, Optional[torch.Tensor]]] = None
                              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """K4 + K7 + K8 of a training step with shared negatives (`bess_neg_score_shared_fwd_loss`): scores [nq, n_neg]
    (K7 applied), loss [], d_pos [nq], d_neg [nq, n_neg].  One launch where the scoring kernel can finish the loss
    rows itself (packed L1 kernel, rows of up to 1024 scores), else the scoring launch + the loss launch(es)."""
    nq, n_neg = int(query.shape[0]), len(neg)
    dev = _neg_operands(d, query, neg, n_neg)
    _same_device([("query", query), ("positive_score", pos), ("triple_weight", weight)])
    _f32(pos, "positive_score")
    _f32(weight, "triple_weight")
    if pos.numel() != nq or weight.numel() not in (1, nq):
        raise ValueError("neg_score_shared_fwd_loss: shapes of positive_score / triple_weight do not match the queries")
    if d.scorer == AFFINE:
        neg, _, _ = _affine_candidates(d, neg)
    # scores, score gradients, row terms, d_pos, loss (dense rows: the backward kernels take contiguous [nq, n_neg]
    # matrices)
    ld = n_neg
    out, dn, row_loss, dp, loss = _carve_f32(dev, nq * ld, nq * ld, nq, nq, 1)
    out, dn = out.view(nq, ld), dn.view(nq, ld)
    ws, ws_bytes = _workspace("bess_neg_score_shared_workspace", d, nq, n_neg, dev)
    kd = _kill_desc(kill, query)
    counters = _counters(dev, (nq + 15) // 16 + 1)
    _launch("bess_neg_score_shared_fwd_loss", dev, ctypes.byref(d), query.data_ptr(), nq, neg.base.data_ptr(),
            _idx(neg.idx, "negative idx"), n_neg, out.data_ptr(), ld, ctypes.byref(kd) if kd is not None else None,
            ctypes.byref(l), pos.data_ptr(), weight.data_ptr(), weight.numel(), row_loss.data_ptr(), loss.data_ptr(),
            dp.data_ptr(), dn.data_ptr(), ld, counters.data_ptr(), _ptr(ws), ws_bytes)
    return out, loss.reshape(()), dp, dn


def scatter_add_rows(dst: torch.Tensor, idx: torch.Tensor, src: torch.Tensor, scale: float = 1.0) -> None:
    dev = _same_device([("dst", dst), ("idx", idx), ("src", src)])
    _f32(dst, "dst")
    _f32(src, "src")
    W = int(dst.shape[1])
    _rows(dst, "dst", W)
    _rows(src, "src", W)
    n = int(src.shape[0])
    ip = _idx(idx, "idx", n)
    _launch("bess_scatter_add_rows", dev, dst.data_ptr(), W, ip, src.data_ptr(), n, scale)


def sparse_sgd(table: torch.Tensor, idx: torch.Tensor, grad: torch.Tensor, lr: float) -> None:
    dev = _same_device([("table", table), ("idx", idx), ("grad", grad)])
    W = int(table.shape[1])
    _rows(table, "table", W)
    _f32(grad, "grad")
    _rows(grad, "grad", W)
    n = int(grad.shape[0])
    ip = _idx(idx, "idx", n)
    _launch("bess_sparse_sgd", dev, _dtype_code(table), W, table.data_ptr(), ip, grad.data_ptr(), n, lr)


def _axpy(axpy: Optional[Tuple[torch.Tensor, torch.Tensor, float]], table: torch.Tensor, who: str
          ) -> Tuple[int, int, int, float]:
    """(table2, grad2, elements, alpha) of the dense `table2 += alpha * grad2` that rides in an update launch, as C
    arguments; (0, 0, 0, 0.0) for None and for an empty table."""
    if axpy is None:
        return 0, 0, 0, 0.0
    x_table, x_grad, x_alpha = axpy
    _same_device([("table", table), ("axpy table", x_table), ("axpy grad", x_grad)])
    _f32(x_grad, "axpy grad")
    if x_table.dtype != table.dtype or not x_table.is_contiguous() or x_grad.numel() != x_table.numel():
        raise ValueError(f"{who}: the axpy table must be contiguous, of the table's dtype, and match its gradient")
    x_n = int(x_table.numel())
    return (x_table.data_ptr() if x_n else 0), (x_grad.data_ptr() if x_n else 0), x_n, float(x_alpha)


def sparse_sgd_lists(table: torch.Tensor, lists: Sequence[Tuple[torch.Tensor, torch.Tensor]], lr: float,
                     axpy: Optional[Tuple[torch.Tensor, torch.Tensor, float]] = None) -> None:
    """`sparse_sgd` for several (row ids, gradient rows) lists in one launch.  `axpy` = (table2, grad2, alpha):
    `table2 += alpha * grad2` (dense, same dtype as `table`) by spare workgroups of the same launch."""
    if not 1 <= len(lists) <= MAX_ROW_LISTS:
        raise ValueError(f"sparse_sgd_lists: {len(lists)} lists (1 .. {MAX_ROW_LISTS})")
    dev = _same_device([("table", table)] + [(f"idx[{i}]", x) for i, (x, _) in enumerate(lists)]
                       + [(f"grad[{i}]", g) for i, (_, g) in enumerate(lists)])
    W = int(table.shape[1])
    _rows(table, "table", W)
    for i, (x, g) in enumerate(lists):
        _f32(g, f"grad[{i}]")
        _rows(g, f"grad[{i}]", W)
        _idx(x, f"idx[{i}]", int(g.shape[0]))
    ip = (_vp * len(lists))(*[x.data_ptr() for x, _ in lists])
    gp = (_vp * len(lists))(*[g.data_ptr() for _, g in lists])
    rows = (_i64 * len(lists))(*[int(g.shape[0]) for _, g in lists])
    _launch("bess_sparse_sgd_lists_axpy", dev, _dtype_code(table), W, table.data_ptr(), len(lists), ip, gp, rows, lr,
            *_axpy(axpy, table, "sparse_sgd_lists"))


def dense_sgd(table: torch.Tensor, grad: torch.Tensor, lr: float) -> None:
    dev = _same_device([("table", table), ("grad", grad)])
    _f32(grad, "grad")
    if not table.is_contiguous() or table.numel() != grad.numel():
        raise ValueError("dense_sgd: table / grad mismatch")
    _launch("bess_dense_sgd", dev, _dtype_code(table), table.data_ptr(), grad.data_ptr(), table.numel(), lr)


SEGMENT_CAP = 256  # BESS_SEGMENT_CAP of include/besskge_hip.h


class SegmentIndex:
    """References grouped by destination row (see bess_build_segment_index)."""

    __slots__ = ("refs", "seg_rows", "seg_offsets", "n_seg", "n_refs", "max_seg", "long_segs", "long_cap", "long_count", "long_grad")

    def __init__(self, idx: torch.Tensor, n_rows: int, width: int = 0,
                 scratch: Optional[dict] = None) -> None:
        """`width` (row width W of the table the gradients are for): lets the scratch of the long-row
        tier be prepared with the index instead of at the first reduction.  `scratch` (a dict the
        caller keeps, e.g. one per model): the zero-initialised scratch of the long-row tier is taken
        from / left in it instead of being allocated and zeroed per index (every use leaves it zero;
        share it only between steps that run one after the other on the same stream)."""
        dev = _dev(idx, "idx")
        ip = _idx(idx, "idx")
        n = int(idx.numel())
        need = ctypes.c_size_t(0)
        _check(load().bess_segment_index_workspace(n, ctypes.byref(need)), "bess_segment_index_workspace")
        ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)
        self._allocate(n, n_rows, dev)
        bits = max(1, int(n_rows - 1).bit_length())
        _launch("bess_build_segment_index", dev, ip, n, bits, self.refs.data_ptr(), self.seg_rows.data_ptr(),
                self.seg_offsets.data_ptr(), self.n_seg.data_ptr(), self.long_segs.data_ptr(), self.long_cap,
                ws.data_ptr(), need.value)
        self._long_scratch(dev, width, scratch)

    def _allocate(self, n: int, n_rows: int, dev: torch.device) -> None:
        # ONE allocation for the index arrays (a notebook-size step builds an index per update: five
        # torch.empty calls were a measurable part of its host time)
        long_cap = n // SEGMENT_CAP + 1
        na, nb = (n + 3) & ~3, (n + 4) & ~3  # every array starts on a 16-byte boundary
        buf = torch.empty((2 * na + nb + 4 + long_cap + 1,), dtype=torch.int32, device=dev)
        self.refs = buf[:n]
        self.seg_rows = buf[na: na + n]
        self.seg_offsets = buf[2 * na: 2 * na + n + 1]
        self.n_seg = buf[2 * na + nb: 2 * na + nb + 1]  # always written by the build
        self.n_refs = n
        self.max_seg = min(n, int(n_rows))
        # rows with more than SEGMENT_CAP references (padded candidate lists, hot entities): listed
        # here, reduced by the whole device instead of one 16-lane group (include/besskge_hip.h)
        self.long_cap = long_cap
        self.long_segs = buf[2 * na + nb + 4:]

    def _long_scratch(self, dev: torch.device, width: int, scratch: Optional[dict]) -> None:
        # scratch of the long-row tier: zero before the first use, left zero / consistent by every use;
        # zeroed here, i.e. on the stream that builds the index (off the critical path of a training step)
        if scratch is not None:
            key = (dev, "long", int(width))
            have = scratch.get(key)
            if have is None or have[0].shape[0] < self.long_cap:
                have = (torch.zeros((self.long_cap,), dtype=torch.int32, device=dev),
                        torch.zeros((self.long_cap, int(width)), dtype=torch.float32, device=dev) if width else None)
                scratch[key] = have
            self.long_count, self.long_grad = have
        else:
            self.long_count = torch.zeros((self.long_cap,), dtype=torch.int32, device=dev)
            self.long_grad = torch.zeros((self.long_cap, int(width)), dtype=torch.float32, device=dev) if width else None


def step_prologue(jobs: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor], int]],
                  id_lists: Sequence[torch.Tensor] = (), n_rows: int = 0, width: int = 0,
                  scratch: Optional[dict] = None) -> Optional[SegmentIndex]:
    """ONE launch in front of a notebook-size training step (`bess_step_prologue`): the copy / fill `jobs`
    (dst, src | None, fill word) over 4-byte elements - dst (and src) contiguous, same number of elements - and
    the segment index of the concatenation of the int32 row-id `id_lists` (read where they are; `n_rows` rows
    in the table they index), returned as a SegmentIndex, or None without lists."""
    if not jobs and not id_lists:
        return None
    if len(jobs) > MAX_WORD_JOBS or len(id_lists) > MAX_ROW_LISTS:
        raise ValueError("step_prologue: too many jobs / id lists")
    tensors = [("job dst", j[0]) for j in jobs] + [("job src", j[1]) for j in jobs] + [("ids", x) for x in id_lists]
    dev = _same_device(tensors)
    nj = len(jobs)
    dst, src, val, words = _job_arrays(jobs, "step_prologue")
    nl = len(id_lists)
    lp, ll = (_vp * max(1, nl))(), (_i64 * max(1, nl))()
    n_ids = 0
    for i, x in enumerate(id_lists):
        if x.dtype != torch.int32 or not x.is_contiguous():
            raise ValueError("step_prologue: id lists must be contiguous int32 tensors")
        lp[i], ll[i] = x.data_ptr(), x.numel()
        n_ids += int(x.numel())
    seg = None
    if nl:
        if not 0 < n_ids <= SMALL_INDEX_MAX:
            raise ValueError(f"step_prologue: {n_ids} row ids (1 .. {SMALL_INDEX_MAX})")
        seg = SegmentIndex.__new__(SegmentIndex)
        seg._allocate(n_ids, n_rows, dev)
    bits = max(1, int(max(1, n_rows) - 1).bit_length())
    _launch("bess_step_prologue", dev, nj, dst, src, val, words, nl, lp, ll, bits, seg.refs.data_ptr() if seg else None,
            seg.seg_rows.data_ptr() if seg else None, seg.seg_offsets.data_ptr() if seg else None,
            seg.n_seg.data_ptr() if seg else None, seg.long_segs.data_ptr() if seg else None,
            seg.long_cap if seg else 0)
    if seg is not None:
        seg._long_scratch(dev, width, scratch)
    return seg


MAX_WORD_JOBS = 8  # BESS_MAX_WORD_JOBS
SMALL_INDEX_MAX = 15360  # BESS_SMALL_INDEX_MAX


class _IdentitySegments:
    """Segments of a table whose every row is updated: row s is segment s."""

    __slots__ = ("seg_rows", "n_seg", "max_seg")

    def __init__(self, n_rows: int, device: torch.device) -> None:
        self.seg_rows = torch.arange(n_rows, dtype=torch.int32, device=device)
        self.n_seg = torch.full((1,), n_rows, dtype=torch.int32, device=device)
        self.max_seg = n_rows


def identity_segments(n_rows: int, device: torch.device) -> _IdentitySegments:
    return _IdentitySegments(n_rows, device)


def neg_pertriple_grad_segments(d: ModelDesc, query: torch.Tensor, table: torch.Tensor, n_neg: int,
                                d_out: torch.Tensor, seg: SegmentIndex,
                                fused_sgd_lr: Optional[float] = None) -> Optional[torch.Tensor]:
    """grad_seg [seg.max_seg, W] f32: one gradient row per unique destination row;
    or, with fused_sgd_lr, apply `table[row] -= lr * grad` in place and return None."""
    dev = _same_device([("query", query), ("table", table), ("d_out", d_out), ("refs", seg.refs)])
    _f32(query, "query")
    _f32(d_out, "d_out")
    _rows(table, "table", d.width)
    nq = int(query.shape[0])
    if _dtype_code(table) != d.dtype or tuple(query.shape) != (nq, query_width(d)) \
            or tuple(d_out.shape) != (nq, n_neg) \
            or seg.n_refs != nq * n_neg:
        raise ValueError("neg_pertriple_grad_segments: operand shapes do not match")
    fused = fused_sgd_lr is not None
    grad = None if fused else torch.empty((seg.max_seg, d.width), dtype=torch.float32, device=dev)
    # (every scorer id has a segmented reduction with a long-row tier)
    if seg.long_grad is None or seg.long_grad.shape[1] != d.width:
        seg.long_grad = torch.zeros((seg.long_cap, d.width), dtype=torch.float32, device=dev)
    _launch("bess_neg_pertriple_grad_segments", dev, ctypes.byref(d), query.data_ptr(), nq, table.data_ptr(), n_neg,
            d_out.data_ptr(), n_neg, seg.refs.data_ptr(), seg.seg_rows.data_ptr(), seg.seg_offsets.data_ptr(),
            seg.n_seg.data_ptr(), seg.max_seg, _ptr(grad), float(fused_sgd_lr) if fused else 0.0,
            seg.long_segs.data_ptr(), seg.long_cap, seg.long_grad.data_ptr(), seg.long_count.data_ptr())
    return grad


def pad_segments(seg: SegmentIndex, grad_seg: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(row ids [max_seg], gradient rows [max_seg, W]) of a segment list with its unused tail neutralised (copies
    of the last real row, zero gradients): an ordinary row list of host-known length - no read-back of n_seg."""
    dev = _same_device([("grad_seg", grad_seg), ("seg_rows", seg.seg_rows)])
    _f32(grad_seg, "grad_seg")
    if grad_seg.dim() != 2 or grad_seg.shape[0] != seg.max_seg or not grad_seg.is_contiguous():
        raise ValueError("pad_segments: grad_seg must be a contiguous [seg.max_seg, W] tensor")
    _launch("bess_pad_segments", dev, seg.seg_rows.data_ptr(), seg.n_seg.data_ptr(), seg.max_seg, grad_seg.data_ptr(),
            int(grad_seg.shape[1]))
    return seg.seg_rows[: seg.max_seg], grad_seg


def apply_segments_sgd(table: torch.Tensor, seg: SegmentIndex, grad_seg: torch.Tensor, lr: float) -> None:
    dev = _same_device([("table", table), ("grad_seg", grad_seg), ("seg_rows", seg.seg_rows)])
    W = int(table.shape[1])
    _rows(table, "table", W)
    _f32(grad_seg, "grad_seg")
    if tuple(grad_seg.shape) != (seg.max_seg, W):
        raise ValueError("apply_segments_sgd: grad_seg shape mismatch")
    _launch("bess_apply_segments_sgd", dev, _dtype_code(table), W, table.data_ptr(), seg.seg_rows.data_ptr(),
            seg.n_seg.data_ptr(), seg.max_seg, grad_seg.data_ptr(), lr)


def segment_sum_rows(src: torch.Tensor, seg: SegmentIndex) -> torch.Tensor:
    """grad_seg [seg.max_seg, W]: rows of `src` [n_refs, W] summed per destination row."""
    dev = _same_device([("src", src), ("refs", seg.refs)])
    _f32(src, "src")
    if src.dim() != 2 or src.shape[0] != seg.n_refs:
        raise ValueError("segment_sum_rows: src must be [n_refs, W]")
    W = int(src.shape[1])
    out = torch.empty((seg.max_seg, W), dtype=torch.float32, device=dev)
    _launch("bess_segment_sum_rows", dev, W, src.data_ptr(), seg.refs.data_ptr(), seg.seg_offsets.data_ptr(),
            seg.n_seg.data_ptr(), seg.max_seg, out.data_ptr())
    return out


def apply_segments_opt(o: OptDesc, table: torch.Tensor, seg: SegmentIndex, grad_seg: torch.Tensor,
                       state1: Optional[torch.Tensor], state2: Optional[torch.Tensor],
                       keep: Optional[torch.Tensor] = None) -> None:
    """`keep` (int32 [seg.max_seg]): update only the segments with a non-zero entry."""
    dev = _same_device([("table", table), ("grad_seg", grad_seg), ("state1", state1), ("state2", state2)])
    W = int(table.shape[1])
    _rows(table, "table", W)
    _f32(grad_seg, "grad_seg")
    if tuple(grad_seg.shape) != (seg.max_seg, W):
        raise ValueError("apply_segments_opt: grad_seg shape mismatch")
    _state_ok(state1, table, o, "state1")
    _state_ok(state2, table, o, "state2")
    _launch("bess_apply_segments_opt", dev, ctypes.byref(o), _dtype_code(table), W, table.data_ptr(),
            seg.seg_rows.data_ptr(), seg.n_seg.data_ptr(), seg.max_seg, grad_seg.data_ptr(), _ptr(state1), _ptr(state2),
            _ptr(keep))


MAX_ROW_LISTS = 8  # BESS_MAX_ROW_LISTS


def coalesced_update(o: Optional[OptDesc], table: torch.Tensor, seg: SegmentIndex, grads: Sequence[torch.Tensor],
                     state1: Optional[torch.Tensor] = None, state2: Optional[torch.Tensor] = None,
                     keep: Optional[torch.Tensor] = None, sum_only: bool = False,
                     axpy: Optional[Tuple[torch.Tensor, torch.Tensor, float]] = None) -> Optional[torch.Tensor]:
    """K9 + K10 of the small lists in one pass: `seg` indexes the concatenation of the lists' row
    ids, `grads[l]` is the f32 [n_l, W] gradient of list l.  Every unique row gets one update
    (one rounding).  `sum_only`: return the per-unique-row sums [seg.max_seg, W] instead.
    `axpy` = (table2, grad2, alpha): `table2 += alpha * grad2` (dense, same dtype as `table`) in the same launch."""
    dev = _same_device([("table", table), ("refs", seg.refs), ("state1", state1), ("state2", state2)]
                       + [(f"grads[{i}]", g) for i, g in enumerate(grads)])
    W = int(table.shape[1])
    _rows(table, "table", W)
    if not 1 <= len(grads) <= MAX_ROW_LISTS:
        raise ValueError(f"coalesced_update: {len(grads)} lists (1 .. {MAX_ROW_LISTS})")
    total = 0
    for i, g in enumerate(grads):
        _f32(g, f"grads[{i}]")
        if g.dim() != 2 or g.shape[1] != W:
            raise ValueError(f"coalesced_update: grads[{i}] must be [n, {W}]")
        total += int(g.shape[0])
    if total != seg.n_refs:
        raise ValueError(f"coalesced_update: the lists hold {total} rows, the index {seg.n_refs} references")
    _state_ok(state1, table, o, "state1")
    _state_ok(state2, table, o, "state2")
    ptrs = (_vp * len(grads))(*[g.data_ptr() for g in grads])
    rows = (_i64 * len(grads))(*[int(g.shape[0]) for g in grads])
    out = torch.empty((seg.max_seg, W), dtype=torch.float32, device=dev) if sum_only else None
    x = _axpy(axpy, table, "coalesced_update")
    _launch("bess_coalesced_update_axpy", dev, ctypes.byref(o) if o is not None else None, _dtype_code(table), W,
            table.data_ptr(), len(grads), ptrs, rows, seg.refs.data_ptr(), seg.seg_rows.data_ptr(),
            seg.seg_offsets.data_ptr(), seg.n_seg.data_ptr(), seg.max_seg, _ptr(state1), _ptr(state2), _ptr(keep),
            _ptr(out), *x)
    return out


class DirectAccumulator:
    """Scratch of `bess_direct_update` for one table: `acc` [M, W] f32 (zero between steps), `claim` [M] int32 (the
    generation of the last step that updated each row), `generation` [1] int32 on the device (incremented once per
    step, before the update: `increment_job()` is the copy job for `step_prologue` that does it)."""

    __slots__ = ("acc", "claim", "generation")

    def __init__(self, table: torch.Tensor) -> None:
        dev = _dev(table, "table")
        self.acc = torch.zeros(tuple(table.shape), dtype=torch.float32, device=dev)
        self.claim = torch.zeros((int(table.shape[0]),), dtype=torch.int32, device=dev)
        self.generation = torch.ones((1,), dtype=torch.int32, device=dev)

    @staticmethod
    def bytes_for(table: torch.Tensor) -> int:
        return int(table.shape[0]) * (int(table.shape[1]) * 4 + 4)

    def increment_job(self) -> Tuple[torch.Tensor, torch.Tensor, int]:
        return (self.generation, self.generation, 1)


def direct_update(o: OptDesc, table: torch.Tensor, id_lists: Sequence[torch.Tensor], scratch: DirectAccumulator,
                  state1: Optional[torch.Tensor] = None, state2: Optional[torch.Tensor] = None,
                  axpy: Optional[Tuple[torch.Tensor, torch.Tensor, float]] = None) -> None:
    """K9 + K10 without an index (`bess_direct_update`): the gradients of the rows named by `id_lists` have been
    added into `scratch.acc` at their row ids; every such row gets ONE optimiser update with its summed gradient,
    its acc row goes back to zero.  `scratch.generation` must have been incremented for this step."""
    dev = _same_device([("table", table), ("acc", scratch.acc), ("state1", state1), ("state2", state2)]
                       + [(f"id_lists[{i}]", x) for i, x in enumerate(id_lists)])
    W = int(table.shape[1])
    _rows(table, "table", W)
    if not 1 <= len(id_lists) <= MAX_ROW_LISTS:
        raise ValueError(f"direct_update: {len(id_lists)} lists (1 .. {MAX_ROW_LISTS})")
    if tuple(scratch.acc.shape) != tuple(table.shape):
        raise ValueError("direct_update: the accumulator belongs to another table")
    for i, x in enumerate(id_lists):
        if x.dtype != torch.int32 or not x.is_contiguous():
            raise ValueError(f"direct_update: id_lists[{i}] must be a contiguous int32 tensor")
    _state_ok(state1, table, o, "state1")
    _state_ok(state2, table, o, "state2")
    ptrs = (_vp * len(id_lists))(*[x.data_ptr() for x in id_lists])
    lens = (_i64 * len(id_lists))(*[int(x.numel()) for x in id_lists])
    _launch("bess_direct_update", dev, ctypes.byref(o), _dtype_code(table), W, table.data_ptr(), len(id_lists), ptrs,
            lens, scratch.acc.data_ptr(), scratch.claim.data_ptr(), scratch.generation.data_ptr(), _ptr(state1),
            _ptr(state2), *_axpy(axpy, table, "direct_update"))


def assign_state_rows(seg: Any, slot_map: torch.Tensor, counter: torch.Tensor, capacity: int,
                      keep: Optional[torch.Tensor] = None) -> None:
    """Paged optimiser state: give the unique rows of `seg` (those with keep != 0) a state row."""
    dev = _same_device([("seg_rows", seg.seg_rows), ("slot_map", slot_map), ("counter", counter), ("keep", keep)])
    if slot_map.dtype != torch.int32 or counter.dtype != torch.int32 or not slot_map.is_contiguous():
        raise ValueError("assign_state_rows: slot_map / counter must be int32")
    _launch("bess_assign_state_rows", dev, seg.seg_rows.data_ptr(), seg.n_seg.data_ptr(), seg.max_seg, _ptr(keep),
            slot_map.data_ptr(), counter.data_ptr(), int(capacity))


def _state_ok(st: Optional[torch.Tensor], table: torch.Tensor, o: Optional[OptDesc], name: str) -> None:
    if st is None:
        return
    _f32(st, name)
    paged = o is not None and o.slot_map != 0
    if st.dim() != 2 or st.shape[1] != table.shape[1] or (not paged and st.shape[0] != table.shape[0]):
        raise ValueError(f"{name} must be [{'capacity' if paged else table.shape[0]}, {table.shape[1]}] float32")


def map_extra_rows(seg: SegmentIndex, extra: SegmentIndex) -> Tuple[torch.Tensor, torch.Tensor]:
    """(extra_map [seg.max_seg], keep [extra.max_seg]) - see bess_neg_pertriple_step_segments."""
    dev = _same_device([("seg_rows", seg.seg_rows), ("extra_rows", extra.seg_rows)])
    xmap = torch.empty((seg.max_seg,), dtype=torch.int32, device=dev)
    keep = torch.empty((extra.max_seg,), dtype=torch.int32, device=dev)
    _launch("bess_map_extra_rows", dev, seg.seg_rows.data_ptr(), seg.n_seg.data_ptr(), seg.max_seg,
            extra.seg_rows.data_ptr(), extra.n_seg.data_ptr(), extra.max_seg, xmap.data_ptr(), keep.data_ptr())
    return xmap, keep


def neg_pertriple_step_segments(d: ModelDesc, query: torch.Tensor, table: torch.Tensor, n_neg: int,
                                d_out: torch.Tensor, seg: SegmentIndex, o: OptDesc,
                                state1: Optional[torch.Tensor], state2: Optional[torch.Tensor],
                                extra_map: Optional[torch.Tensor] = None,
                                extra_sum: Optional[torch.Tensor] = None) -> None:
    """K9 + K10 in one pass: optimiser `o` applied to the unique rows of `seg` with their summed
    gradient (+ extra_sum[extra_map[s]]), in place (TransE / RotatE / DistMult / ComplEx)."""
    dev = _same_device([("query", query), ("table", table), ("d_out", d_out), ("refs", seg.refs),
                        ("state1", state1), ("state2", state2), ("extra_sum", extra_sum)])
    _f32(query, "query")
    _f32(d_out, "d_out")
    _rows(table, "table", d.width)
    nq = int(query.shape[0])
    if _dtype_code(table) != d.dtype or tuple(query.shape) != (nq, query_width(d)) \
            or tuple(d_out.shape) != (nq, n_neg) or seg.n_refs != nq * n_neg:
        raise ValueError("neg_pertriple_step_segments: operand shapes do not match")
    _state_ok(state1, table, o, "state1")
    _state_ok(state2, table, o, "state2")
    if (extra_map is None) != (extra_sum is None):
        raise ValueError("neg_pertriple_step_segments: extra_map and extra_sum come together")
    if extra_sum is not None:
        _f32(extra_sum, "extra_sum")
        if extra_sum.shape[1] != d.width or extra_map.dtype != torch.int32 or extra_map.numel() != seg.max_seg:
            raise ValueError("neg_pertriple_step_segments: extra_map / extra_sum shapes")
    if seg.long_grad is None or seg.long_grad.shape[1] != d.width:
        seg.long_grad = torch.zeros((seg.long_cap, d.width), dtype=torch.float32, device=dev)
    _launch("bess_neg_pertriple_step_segments", dev, ctypes.byref(d), query.data_ptr(), nq, table.data_ptr(), n_neg,
            d_out.data_ptr(), n_neg, seg.refs.data_ptr(), seg.seg_rows.data_ptr(), seg.seg_offsets.data_ptr(),
            seg.n_seg.data_ptr(), seg.max_seg, seg.long_segs.data_ptr(), seg.long_cap, seg.long_grad.data_ptr(),
            seg.long_count.data_ptr(), ctypes.byref(o), _ptr(state1), _ptr(state2), _ptr(extra_map), _ptr(extra_sum))


def ranks_from_scores(pos: torch.Tensor, cand: torch.Tensor, mode: int, worst_rank_infty: bool) -> torch.Tensor:
    dev = _same_device([("pos_score", pos), ("candidate_score", cand)])
    pos = pos.reshape(-1).float().contiguous()
    cand = cand.float().contiguous()
    if cand.dim() != 2 or cand.shape[0] != pos.numel():
        raise ValueError("`pos_score` and `candidate_score` need to have same size at dimension 0")
    out = torch.empty((pos.numel(),), dtype=torch.float32, device=dev)
    _launch("bess_ranks_from_scores", dev, pos.data_ptr(), cand.data_ptr(), pos.numel(), cand.shape[1], cand.shape[1],
            mode, int(worst_rank_infty), out.data_ptr())
    return out


def ranks_from_indices(truth: torch.Tensor, cand: torch.Tensor, worst_rank_infty: bool) -> torch.Tensor:
    dev = _same_device([("ground_truth", truth), ("candidate_indices", cand)])
    truth = truth.reshape(-1).to(torch.int64).contiguous()
    cand = cand.to(torch.int64).contiguous()
    if cand.dim() != 2 or cand.shape[0] != truth.numel():
        raise ValueError("`ground_truth` and `candidate_indices` need to have the same size for dimension 0")
    out = torch.empty((truth.numel(),), dtype=torch.float32, device=dev)
    _launch("bess_ranks_from_indices", dev, truth.data_ptr(), cand.data_ptr(), truth.numel(), cand.shape[1],
            int(worst_rank_infty), out.data_ptr())
    return out


_TOPK_FLAGS = "flags must be a contiguous uint8 [rows, 4 * ceil(L / 256)] tensor"


def _topk(who: str, ordered: bool, scores: torch.Tensor, best_score: torch.Tensor, best_id: torch.Tensor,
          ids: Optional[torch.Tensor], id_base: int, mask: Optional[torch.Tensor], flags: Optional[torch.Tensor],
          excl_ptr: Optional[torch.Tensor] = None, excl_ids: Optional[torch.Tensor] = None,
          round_f16: bool = False) -> None:
    """The checks and the launch of `topk_update` (`ordered` False) and `topk_update_excl` (True); `who`: the name
    in the messages."""
    dev = _same_device([("scores", scores), ("best_score", best_score), ("best_id", best_id), ("ids", ids),
                        ("mask", mask), ("flags", flags), ("excl_ptr", excl_ptr), ("excl_ids", excl_ids)])
    if scores.dtype != torch.float32 or scores.dim() != 2 or (scores.shape[1] > 1 and scores.stride(1) != 1):
        raise ValueError(f"{who}: scores must be float32 [rows, L] with contiguous rows")
    _f32(best_score, "best_score")
    if best_score.dim() != 2 or best_score.shape[0] != scores.shape[0] \
            or best_id.shape != best_score.shape or best_id.dtype != torch.int32 or not best_id.is_contiguous():
        raise ValueError(f"{who}: best lists must be [rows, kk] (f32 scores, int32 ids)")
    R, L, kk = int(scores.shape[0]), int(scores.shape[1]), int(best_score.shape[1])
    if (excl_ptr is None) != (excl_ids is None):
        raise ValueError(f"{who}: excl_ptr and excl_ids go together")
    ep = ei = n_excl = 0
    if excl_ptr is not None:
        for t in (excl_ptr, excl_ids):
            if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
                raise ValueError(f"{who}: excl_ptr / excl_ids must be contiguous 1-D int32 tensors")
        if excl_ptr.numel() != R + 1:
            raise ValueError(f"{who}: excl_ptr has {excl_ptr.numel()} entries, expected rows + 1 = {R + 1}")
        ep, ei, n_excl = excl_ptr.data_ptr(), excl_ids.data_ptr(), int(excl_ids.numel())
    ip, ir, _ = _mat(ids, torch.int32, "ids must be a contiguous int32 [1 | rows, L] tensor", (1, R), L, who)
    mp, mr, _ = _mat(mask, torch.bool, "mask must be a contiguous bool [1 | rows, L] tensor", (1, R), L, who)
    ld = int(scores.stride(0)) if R > 1 else L
    if flags is None:
        if ordered:
            _launch("bess_topk_update_excl", dev, scores.data_ptr(), R, L, max(ld, L), ip, ir, int(id_base), mp, mr, ep,
                    ei, n_excl, int(bool(round_f16)), best_score.data_ptr(), best_id.data_ptr(), kk)
        else:
            _launch("bess_topk_update", dev, scores.data_ptr(), R, L, max(ld, L), ip, ir, int(id_base), mp, mr,
                    best_score.data_ptr(), best_id.data_ptr(), kk)
        return
    if mask is not None or (ids is not None and (ir != 1 or not ordered)):
        raise ValueError(f"{who}: flagged tiles take one shared row of ids (or id_base) and no mask" if ordered
                         else f"{who}: flagged tiles take ids from id_base and no mask")
    fp, _, fc = _mat(flags, torch.uint8, _TOPK_FLAGS, (R,), None, who)
    if fc % 4 or fc * 64 < L:
        raise ValueError(f"{who}: {_TOPK_FLAGS}")
    if ordered:
        _launch("bess_topk_update_flagged_excl", dev, scores.data_ptr(), R, L, max(ld, L), fp, fc, ip, int(id_base), ep,
                ei, n_excl, int(bool(round_f16)), best_score.data_ptr(), best_id.data_ptr(), kk)
    else:
        _launch("bess_topk_update_flagged", dev, scores.data_ptr(), R, L, max(ld, L), fp, fc, int(id_base),
                best_score.data_ptr(), best_id.data_ptr(), kk)


def topk_update(scores: torch.Tensor, best_score: torch.Tensor, best_id: torch.Tensor,
                ids: Optional[torch.Tensor] = None, id_base: int = 0, mask: Optional[torch.Tensor] = None,
                flags: Optional[torch.Tensor] = None) -> None:
    """Merge `scores` [rows, L] into the running (best_score, best_id) [rows, kk] lists in place.
    `flags` (from `neg_score_shared_fwd_pruned`): only the flagged blocks of 64 columns are read."""
    _topk("topk_update", False, scores, best_score, best_id, ids, id_base, mask, flags)


#: id of an empty entry of the ordered lists (`topk_update_excl`): nothing sorts after (-inf, TOPK_ID_NONE)
TOPK_ID_NONE = 2**31 - 1


def topk_update_excl(scores: torch.Tensor, best_score: torch.Tensor, best_id: torch.Tensor,
                     ids: Optional[torch.Tensor] = None, id_base: int = 0, mask: Optional[torch.Tensor] = None,
                     flags: Optional[torch.Tensor] = None, excl_ptr: Optional[torch.Tensor] = None,
                     excl_ids: Optional[torch.Tensor] = None, round_f16: bool = False) -> None:
    """`topk_update` under the total order (score descending, id ascending), leaving out the candidates named by
    the rows' exclusion lists (`bess_topk_update_excl` / `bess_topk_update_flagged_excl`): the result does not
    depend on the order of columns, tiles or shards.  Lists start out as (-inf, TOPK_ID_NONE).

    `excl_ptr` [rows + 1], `excl_ids` (int32, CSR; ids ascending within a row, in the id space of the candidates).
    `round_f16`: scores are rounded to fp16 before they are compared and stored.  With `flags`, `ids` is one row
    [1, L] shared by all rows (or None: `id_base` + column) and there is no mask; the thresholds the tile was
    pruned with must be strictly below the rows' kk-th scores."""
    _topk("topk_update_excl", True, scores, best_score, best_id, ids, id_base, mask, flags, excl_ptr, excl_ids, round_f16)


# --------------------------------------------------------------------------- #
# device-side index sampling
def _int_tensor(t: Optional[torch.Tensor], name: str, dtype: torch.dtype, numel: Optional[int] = None) -> int:
    if t is None:
        return 0
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"`{name}` must be contiguous {dtype}, got {t.dtype}")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"`{name}` has {t.numel()} elements, expected {numel}")
    return t.data_ptr()


def sample_negatives(gen: Pcg64State, jump_table: torch.Tensor, n_step: int, n_shard: int, src_begin: int,
                     src_count: int, B: int, K: int, shard_counts: torch.Tensor,
                     wanted_type: Optional[torch.Tensor] = None, type_counts: Optional[torch.Tensor] = None,
                     type_offsets: Optional[torch.Tensor] = None, local_sampling: bool = False) -> torch.Tensor:
    dev = _same_device([("jump_table", jump_table), ("shard_counts", shard_counts), ("wanted_type", wanted_type),
                        ("type_counts", type_counts), ("type_offsets", type_offsets)])
    tp = _int_tensor(jump_table, "jump_table", torch.int64, 64 * 4)
    cp = _int_tensor(shard_counts, "shard_counts", torch.int32, n_shard)
    n_type = 0
    if wanted_type is not None:
        if type_counts is None or type_offsets is None or type_counts.shape != type_offsets.shape \
                or type_counts.dim() != 2 or type_counts.shape[0] != n_shard:
            raise ValueError("type tables must both be [n_shard, n_type]")
        n_type = int(type_counts.shape[1])
    wp = _int_tensor(wanted_type, "wanted_type", torch.int32, n_step * n_shard * B)
    tcp = _int_tensor(type_counts, "type_counts", torch.int32)
    top = _int_tensor(type_offsets, "type_offsets", torch.int32)
    out = torch.empty((n_step, src_count, n_shard, B, K), dtype=torch.int32, device=dev)
    _launch("bess_sample_negatives", dev, ctypes.byref(gen), tp, n_step, n_shard, src_begin, src_count, B, K, cp, wp, tcp,
            top, n_type, int(local_sampling), out.data_ptr())
    return out


def sample_negatives_weighted(gen: Pcg64State, jump_table: torch.Tensor, n_step: int, n_shard: int, src_begin: int,
                              src_count: int, B: int, K: int, cum_weights: torch.Tensor,
                              shard_counts: torch.Tensor) -> torch.Tensor:
    """`WeightedShardedNegativeSampler.__call__` for source shards [src_begin, src_begin + src_count): int32
    [n_step, src_count, n_shard, B, K].  cum_weights int64 [src_count, ld]: the running sums of those shards' rows
    (row s - src_begin for shard s); shard_counts int32 [n_shard]."""
    dev = _same_device([("jump_table", jump_table), ("cum_weights", cum_weights), ("shard_counts", shard_counts)])
    tp = _int_tensor(jump_table, "jump_table", torch.int64, 64 * 4)
    cp = _int_tensor(shard_counts, "shard_counts", torch.int32, n_shard)
    if src_begin < 0 or src_count < 0 or src_begin + src_count > n_shard:
        raise ValueError(f"source shards [{src_begin}, {src_begin + src_count}) outside {n_shard} shards")
    if cum_weights.dim() != 2 or cum_weights.shape[0] != src_count or cum_weights.shape[1] < 1:
        raise ValueError(f"`cum_weights` must be [src_count = {src_count}, ld >= 1], got {tuple(cum_weights.shape)}")
    wp = _int_tensor(cum_weights, "cum_weights", torch.int64)
    out = torch.empty((n_step, src_count, n_shard, B, K), dtype=torch.int32, device=dev)
    _launch("bess_sample_negatives_weighted", dev, ctypes.byref(gen), tp, n_step, n_shard, src_begin, src_count, B, K, wp,
            int(cum_weights.shape[1]), cp, out.data_ptr())
    return out


def gather_negative_logq(negatives: torch.Tensor, log_q: torch.Tensor, src_begin: int, dst_begin: int, dst_count: int,
                         local_sampling: bool) -> torch.Tensor:
    """Log-proposals of drawn negatives in the layout of their scores (`bess_gather_negative_logq`): negatives int32
    [n_step, src_count, n_shard, B, K] (source shards from `src_begin`), log_q float32 [n_shard, ld] -> float32
    [n_step, dst_count, B, n_shard, K] for scoring shards [dst_begin, dst_begin + dst_count)."""
    dev = _same_device([("negatives", negatives), ("log_q", log_q)])
    if negatives.dim() != 5 or log_q.dim() != 2 or log_q.shape[0] != negatives.shape[2] or log_q.shape[1] < 1:
        raise ValueError(f"negatives must be [n_step, src_count, n_shard, B, K] and log_q [n_shard, ld >= 1], got "
                         f"{tuple(negatives.shape)} and {tuple(log_q.shape)}")
    n_step, src_count, n, B, K = (int(x) for x in negatives.shape)
    np_ = _int_tensor(negatives, "negatives", torch.int32)
    _f32(log_q, "log_q")
    out = torch.empty((n_step, dst_count, B, n, K), dtype=torch.float32, device=dev)
    _launch("bess_gather_negative_logq", dev, np_, log_q.data_ptr(), int(log_q.shape[1]), n_step, n, src_begin,
            src_count, dst_begin, dst_count, B, K, int(local_sampling), out.data_ptr())
    return out


def sample_bucket_indices(gen: Pcg64State, jump_table: torch.Tensor, shape: Sequence[int], counts: torch.Tensor,
                          offsets: torch.Tensor) -> torch.Tensor:
    """`offsets + rng.integers(1 << 63, size=shape) % counts` with counts / offsets
    broadcast over shape[1:-1] (shape = [step, buckets..., inner])."""
    dev = _same_device([("jump_table", jump_table), ("counts", counts), ("offsets", offsets)])
    tp = _int_tensor(jump_table, "jump_table", torch.int64, 64 * 4)
    n_bucket = 1
    for s in shape[1:-1]:
        n_bucket *= int(s)
    cp = _int_tensor(counts, "counts", torch.int64, n_bucket)
    op = _int_tensor(offsets, "offsets", torch.int64, n_bucket)
    out = torch.empty(tuple(int(s) for s in shape), dtype=torch.int64, device=dev)
    _launch("bess_sample_bucket_indices", dev, ctypes.byref(gen), tp, out.numel(), int(shape[-1]), n_bucket, cp, op,
            out.data_ptr())
    return out


def lookup_triples(triples: torch.Tensor, sample_idx: torch.Tensor, swap_tail: bool,
                   want: Sequence[str] = ("head", "relation", "tail")) -> dict:
    """head / relation / tail (int32) of the sampled triples; sample_idx is
    [step, n, ppp] or [step, n, n, ppp]; the tail is block-transposed when swap_tail."""
    dev = _same_device([("triples", triples), ("sample_idx", sample_idx)])
    if triples.dtype != torch.int32 or triples.dim() != 2 or triples.shape[1] != 3 or not triples.is_contiguous():
        raise ValueError("`triples` must be a contiguous int32 [n_triple, 3] tensor")
    _int_tensor(sample_idx, "sample_idx", torch.int64)
    if sample_idx.dim() == 3:
        n_step, n1, ppp = sample_idx.shape
        n2 = 1
    elif sample_idx.dim() == 4:
        n_step, n1, n2, ppp = sample_idx.shape
    else:
        raise ValueError("`sample_idx` must be [step, n, ppp] or [step, n, n, ppp]")
    if swap_tail and sample_idx.dim() != 4:
        raise ValueError("the tail transpose needs shard-pair buckets")
    out = {}
    for k in want:
        shape = tuple(sample_idx.shape)
        if k == "tail" and swap_tail:
            shape = (n_step, n2, n1, ppp)
        out[k] = torch.empty(shape, dtype=torch.int32, device=dev)
    ptr = lambda k: out[k].data_ptr() if k in out else 0  # noqa: E731
    _launch("bess_lookup_triples", dev, triples.data_ptr(), triples.shape[0], sample_idx.data_ptr(), n_step, n1, n2, ppp,
            int(swap_tail), ptr("head"), ptr("relation"), ptr("tail"))
    return out


def gather_candidate_lists(table_h: torch.Tensor, mask_h: Optional[torch.Tensor], lookup: torch.Tensor,
                           table_t: Optional[torch.Tensor] = None, mask_t: Optional[torch.Tensor] = None,
                           per_part: int = 1, half: int = 1, mask_gather_layout: bool = False,
                           want_mask: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Fixed candidate lists of the sampled triples, laid out for the exchange (see
    bess_gather_candidate_lists): tables int32 [n_list, n_neg_shard, L] (+ bool masks), lookup int64
    [n_step, n_shard, T] -> (entities int32 [n_step, n_neg_shard, n_shard, T, L], mask bool | None)."""
    dev = _same_device([("table_h", table_h), ("mask_h", mask_h), ("lookup", lookup), ("table_t", table_t),
                        ("mask_t", mask_t)])
    for t, nm in ((table_h, "table_h"), (table_t, "table_t")):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 3 or not t.is_contiguous()):
            raise ValueError(f"`{nm}` must be a contiguous int32 [n_list, n_neg_shard, L] tensor")
    for t, nm in ((mask_h, "mask_h"), (mask_t, "mask_t")):
        if t is not None and (t.dtype != torch.bool or tuple(t.shape) != tuple(table_h.shape) or not t.is_contiguous()):
            raise ValueError(f"`{nm}` must be a contiguous bool tensor of the tables' shape")
    if table_t is not None and tuple(table_t.shape) != tuple(table_h.shape):
        raise ValueError("the two candidate tables must have the same shape")
    if lookup.dtype != torch.int64 or lookup.dim() != 3 or not lookup.is_contiguous():
        raise ValueError("`lookup` must be a contiguous int64 [n_step, n_shard, T] tensor")
    n_list, n_neg_shard, L = (int(x) for x in table_h.shape)
    n_step, n_shard, T = (int(x) for x in lookup.shape)
    ent = torch.empty((n_step, n_neg_shard, n_shard, T, L), dtype=torch.int32, device=dev)
    msk = None
    if want_mask and mask_h is not None:
        shape = (n_step, n_neg_shard, n_shard, T, L) if mask_gather_layout else (n_step, n_shard, T, n_neg_shard, L)
        msk = torch.empty(shape, dtype=torch.bool, device=dev)
    _launch("bess_gather_candidate_lists", dev, table_h.data_ptr(), _ptr(table_t), _ptr(mask_h), _ptr(mask_t), n_list,
            lookup.data_ptr(), n_step, n_shard, T, int(per_part), int(half), n_neg_shard, L,
            int(bool(mask_gather_layout)), ent.data_ptr(), _ptr(msk))
    return ent, msk


def _index_ptrs(ix: Optional[Sequence[torch.Tensor]], name: str) -> Tuple[int, int, int, int]:
    """(keys, offsets, n_pair, completions) of one side of a `KnownTripleFilter` index, as C arguments."""
    if ix is None:
        return 0, 0, 0, 0
    keys, off, comp = ix
    n_pair = int(keys.numel())
    _int_tensor(keys, f"{name} keys", torch.int64)
    _int_tensor(off, f"{name} offsets", torch.int64, n_pair + 1)
    _int_tensor(comp, f"{name} completions", torch.int32)
    return keys.data_ptr(), off.data_ptr(), n_pair, comp.data_ptr()


def _known_rows(index: Sequence[torch.Tensor], index2: Optional[Sequence[torch.Tensor]], kept: torch.Tensor,
                relation: torch.Tensor, side: Optional[torch.Tensor], kept_shard: Optional[torch.Tensor],
                local_to_global: Optional[torch.Tensor]) -> Tuple[Any, ...]:
    """The leading C arguments that `bess_known_triple_mask` and `bess_known_completions` share, in their order - the
    two indices, kept, kept_shard, relation, side, n_row, the row count itself - and then (map, ld_map, n_map_shard)
    of `local_to_global`, which the two take further back."""
    n_row = int(kept.numel())
    kp = _int_tensor(kept, "kept", torch.int32)
    rp = _int_tensor(relation, "relation", torch.int32, n_row)
    ksp = _int_tensor(kept_shard, "kept_shard", torch.int32, n_row)
    sp = 0
    if side is not None:
        if side.dtype not in (torch.uint8, torch.bool) or not side.is_contiguous() or side.numel() != n_row:
            raise ValueError(f"`side` must be contiguous uint8 / bool with {n_row} entries")
        if index2 is None:
            raise ValueError("a `side` vector needs the index of both sides (`index2`)")
        sp = side.data_ptr()
    mp, n_map_shard, ld_map = _mat(local_to_global, torch.int32,
                                   "`local_to_global` must be a contiguous int32 [n_shard, rows per shard] tensor")
    if local_to_global is None and kept_shard is not None:
        raise ValueError("`kept_shard` needs `local_to_global`")
    return (*_index_ptrs(index, "index"), *_index_ptrs(index2, "index2"), kp, ksp, rp, sp, n_row), (mp, ld_map, n_map_shard)


def known_triple_mask(index: Sequence[torch.Tensor], kept: torch.Tensor, relation: torch.Tensor, cand: torch.Tensor,
                      mask: torch.Tensor, n_relation: int, index2: Optional[Sequence[torch.Tensor]] = None,
                      side: Optional[torch.Tensor] = None, kept_shard: Optional[torch.Tensor] = None,
                      n_col: Optional[int] = None, ld_cand: Optional[int] = None, n_cand_row: Optional[int] = None,
                      cand_row: Optional[torch.Tensor] = None, cols_per_block: int = 0, block_stride: int = 0,
                      cand_shard: int = -1, local_to_global: Optional[torch.Tensor] = None,
                      ld_mask: Optional[int] = None, and_into: bool = False) -> torch.Tensor:
    """mask[i, j] = 0 where (kept_i, relation_i, cand_ij) is a known triple, 1 elsewhere (bess_known_triple_mask;
    with `and_into` bytes are only cleared).  `index` / `index2`: (pair keys int64 [P], offsets int64 [P + 1],
    completions int32) of `KnownTripleFilter`; rows take `index2` where `side` (uint8 / bool [rows]) is set.
    `cand`: int32 [rows, columns], or flat with the geometry given (`n_col`, `ld_cand`, `n_cand_row`, blocks of
    `cols_per_block` columns `block_stride` apart); `mask`: uint8 / bool [rows, ld_mask], or flat with `ld_mask`."""
    dev = _same_device([("kept", kept), ("relation", relation), ("cand", cand), ("mask", mask), ("side", side),
                        ("kept_shard", kept_shard), ("cand_row", cand_row), ("local_to_global", local_to_global),
                        *[(f"index[{k}]", t) for k, t in enumerate(index)],
                        *[(f"index2[{k}]", t) for k, t in enumerate(index2 or ())]])
    rows, l2g = _known_rows(index, index2, kept, relation, side, kept_shard, local_to_global)
    n_row = rows[-1]
    crp = _int_tensor(cand_row, "cand_row", torch.int32, n_row)
    _int_tensor(cand, "cand", torch.int32)
    if cand.dim() == 2 and n_col is None:
        n_cand_row, n_col = (int(x) for x in cand.shape)
        ld_cand = n_col if ld_cand is None else ld_cand
    if n_col is None or ld_cand is None or n_cand_row is None:
        raise ValueError("a flat `cand` needs `n_col`, `ld_cand` and `n_cand_row`")
    n_col, ld_cand, n_cand_row = int(n_col), int(ld_cand), int(n_cand_row)
    cpb = int(cols_per_block) if cols_per_block > 0 else max(n_col, 1)
    stride = int(block_stride) if cols_per_block > 0 else cpb
    empty = n_row == 0 or n_col == 0  # (nothing is read or written then)
    if n_col < 0 or ld_cand < 0 or stride < cpb or (n_cand_row < 1 and not empty):
        raise ValueError("bad candidate geometry")
    n_block = -(-n_col // cpb)
    span = (n_block - 1) * stride + (n_col - (n_block - 1) * cpb)  # elements from a candidate row's start to its end
    if not empty and (n_cand_row - 1 if ld_cand else 0) * ld_cand + span > cand.numel():
        raise ValueError(f"`cand` has {cand.numel()} elements, the geometry given reaches past them")
    if not empty and ld_cand and cand_row is None and n_cand_row < n_row:
        raise ValueError(f"{n_cand_row} candidate rows for {n_row} rows")
    if mask.dtype not in (torch.uint8, torch.bool) or not mask.is_contiguous():
        raise ValueError("`mask` must be contiguous uint8 / bool")
    if ld_mask is None:
        if mask.dim() != 2:
            raise ValueError("a flat `mask` needs `ld_mask`")
        ld_mask = int(mask.shape[1])
    ld_mask = int(ld_mask)
    if ld_mask < n_col or (n_row > 0 and n_col > 0 and (n_row - 1) * ld_mask + n_col > mask.numel()):
        raise ValueError(f"`mask` ({mask.numel()} bytes, ld {ld_mask}) does not hold {n_row} x {n_col}")
    if local_to_global is not None and (cand_shard >= l2g[2] or (cand_shard < 0 and n_block > l2g[2])):
        raise ValueError("`local_to_global` does not cover the candidates' shards")
    _launch("bess_known_triple_mask", dev, *rows, int(n_relation), cand.data_ptr(), n_col, ld_cand, n_cand_row, crp, cpb,
            stride, int(cand_shard), *l2g, mask.data_ptr(), ld_mask, int(bool(and_into)))
    return mask


def known_completions(index: Sequence[torch.Tensor], kept: torch.Tensor, relation: torch.Tensor, n_relation: int,
                      index2: Optional[Sequence[torch.Tensor]] = None, side: Optional[torch.Tensor] = None,
                      kept_shard: Optional[torch.Tensor] = None, local_to_global: Optional[torch.Tensor] = None,
                      skip: Optional[torch.Tensor] = None, keep_entity: Optional[torch.Tensor] = None,
                      counts: Optional[torch.Tensor] = None, dst: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None, out_stride: int = 1,
                      tag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One pass of bess_known_completions over the rows (kept_i, relation_i[, side_i]) of the index of
    `known_triple_mask`.  Count pass (`counts` int32 [rows]): counts[i] = known completions of row i that are not
    `skip[i]` (int32 [rows], -1: none) and whose `keep_entity` byte (uint8 / bool [n_entity]) is set.  Fill pass
    (`dst` int64 [rows], `out` int32 with a multiple of `out_stride` elements): the k-th of them, ascending, goes to
    out.view(-1, out_stride)[dst[i] + k, -1], and with `out_stride` 2 `tag[i]` to [dst[i] + k, 0].  Returns the
    tensor written."""
    dev = _same_device([("kept", kept), ("relation", relation), ("side", side), ("kept_shard", kept_shard),
                        ("local_to_global", local_to_global), ("skip", skip), ("keep_entity", keep_entity),
                        ("counts", counts), ("dst", dst), ("out", out), ("tag", tag),
                        *[(f"index[{k}]", t) for k, t in enumerate(index)],
                        *[(f"index2[{k}]", t) for k, t in enumerate(index2 or ())]])
    rows, l2g = _known_rows(index, index2, kept, relation, side, kept_shard, local_to_global)
    n_row = rows[-1]
    skp = _int_tensor(skip, "skip", torch.int32, n_row)
    kep, n_entity = 0, 0
    if keep_entity is not None:
        if keep_entity.dtype not in (torch.uint8, torch.bool) or not keep_entity.is_contiguous():
            raise ValueError("`keep_entity` must be contiguous uint8 / bool")
        kep, n_entity = keep_entity.data_ptr(), int(keep_entity.numel())
    if (counts is None) == (dst is None and out is None):
        raise ValueError("exactly one pass per call: `counts`, or `dst` and `out`")
    cp = _int_tensor(counts, "counts", torch.int32, n_row)
    dp = _int_tensor(dst, "dst", torch.int64, n_row)
    op, n_out = 0, 0
    if counts is None:
        if dst is None or out is None:
            raise ValueError("the fill pass needs `dst` and `out`")
        if out_stride not in (1, 2) or (out_stride == 2 and tag is None):
            raise ValueError("`out_stride` is 1, or 2 with a `tag` vector")
        op = _int_tensor(out, "out", torch.int32)
        if out.numel() % out_stride:
            raise ValueError(f"`out` has {out.numel()} elements: not a multiple of out_stride {out_stride}")
        n_out = out.numel() // out_stride
    tp = _int_tensor(tag, "tag", torch.int32, n_row)
    _launch("bess_known_completions", dev, *rows, int(n_relation), *l2g, skp, kep, n_entity, cp, dp, op, n_out,
            int(out_stride), tp)
    return counts if counts is not None else out  # type: ignore[return-value]


# --------------------------------------------------------------------------- #
# collectives between shards (RCCL through the C ABI)
def comm_unique_id() -> bytes:
    """128 opaque bytes; made by one rank, handed to every rank's `Communicator`."""
    buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
    _check(load().bess_comm_unique_id(buf), "bess_comm_unique_id")
    return bytes(buf)


class Communicator:
    """`bess_comm*` of this rank (owns it: destroyed with the object).  Belongs to the HIP
    device that is current when it is made; collectives run on PyTorch's current stream
    of that device."""

    def __init__(self, world: int, rank: int, unique_id: bytes, device: torch.device) -> None:
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError(f"unique id must be {COMM_ID_BYTES} bytes")
        if device.type != "cuda":
            raise RuntimeError("besskge: communicators live on HIP devices (there is no CPU fallback)")
        self.world, self.rank, self.device = int(world), int(rank), device
        self._h = _vp()
        buf = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        with torch.cuda.device(device):
            _check(load().bess_comm_init_rank(self.world, self.rank, buf, ctypes.byref(self._h)),
                   "bess_comm_init_rank")

    @classmethod
    def init_all(cls, devices: Sequence[torch.device]) -> List["Communicator"]:
        """One process driving several GPUs (`bess_comm_init_all` = ncclCommInitAll): communicator r of the
        clique lives on `devices[r]`.  Collectives of the clique's ranks must be issued from different host
        threads or inside one RCCL group; with one device it is a self-contained one-rank communicator."""
        n = len(devices)
        if n < 1 or any(d.type != "cuda" for d in devices):
            raise RuntimeError("besskge: communicators live on HIP devices (there is no CPU fallback)")
        ids = (ctypes.c_int32 * n)(*[d.index if d.index is not None else torch.cuda.current_device() for d in devices])
        handles = (_vp * n)()
        _check(load().bess_comm_init_all(n, ids, handles), "bess_comm_init_all")
        out = []
        for r, d in enumerate(devices):
            c = cls.__new__(cls)
            c.world, c.rank, c.device = n, r, torch.device("cuda", int(ids[r]))
            c._h = _vp(handles[r])
            out.append(c)
        return out

    def info(self) -> Tuple[int, int, int]:
        """(world, rank, device index) as the library holds them (`bess_comm_info`)."""
        w, r, d = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(load().bess_comm_info(self._h, ctypes.byref(w), ctypes.byref(r), ctypes.byref(d)), "bess_comm_info")
        return w.value, r.value, d.value

    def close(self) -> None:
        """`bess_comm_destroy`.  `ncclCommDestroy` waits for hipGraphs that recorded collectives of this
        communicator, so they must be destroyed first: a communicator that has seen one of its collectives
        recorded refuses to be destroyed until `graphs_released()` says they are gone (`NativeGroup.close()`
        does both, in order) - an error instead of a process that never ends."""
        if getattr(self, "_h", None) is not None and self._h.value:
            if getattr(self, "_recorded", False):
                raise RuntimeError(
                    "besskge: this communicator's collectives were recorded into a hipGraph; destroy the graphs "
                    "(NativeGroup.close() / ReplicaGroup.release_graphs()) and call graphs_released() first - "
                    "ncclCommDestroy would wait for them forever")
            torch.cuda.synchronize(self.device)
            h, self._h = self._h, _vp()
            _check(load().bess_comm_destroy(h), "bess_comm_destroy")

    def graphs_released(self) -> None:
        """The caller has destroyed every hipGraph that recorded this communicator's collectives."""
        self._recorded = False

    def _note_capture(self) -> None:
        if not getattr(self, "_recorded", False) and torch.cuda.is_current_stream_capturing():
            self._recorded = True

    def __del__(self, _finalizing: Any = sys.is_finalizing) -> None:  # pragma: no cover - shutdown order
        # Never `ncclCommDestroy` from a finaliser that cannot know the graphs are gone: at interpreter shutdown
        # (objects die in no useful order) or when a collective was recorded and nobody released the graphs, the
        # handle is left to the process teardown.
        if _finalizing() or getattr(self, "_recorded", False):
            return
        try:
            self.close()
        except Exception:
            pass

    def _buf(self, t: torch.Tensor, name: str) -> int:
        if not t.is_cuda or t.device != self.device:
            raise RuntimeError(f"besskge: `{name}` is on {t.device}, the communicator on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"`{name}` must be contiguous")
        return t.data_ptr()

    def all_to_all(self, send: torch.Tensor, recv: Optional[torch.Tensor] = None) -> torch.Tensor:
        """send [world, ...]: block p goes to rank p; returns recv (block p came from rank p)."""
        if send.dim() < 1 or send.shape[0] != self.world:
            raise ValueError(f"all_to_all: leading dim {tuple(send.shape)[:1]} != world {self.world}")
        if recv is None:
            recv = torch.empty_like(send)
        elif recv.shape != send.shape or recv.dtype != send.dtype:
            raise ValueError("all_to_all: recv does not match send")
        per_peer = send[0].numel() * send.element_size()
        self._note_capture()
        _launch("bess_alltoall", self.device, self._h, self._buf(send, "send"), self._buf(recv, "recv"), per_peer)
        return recv

    def all_gather(self, send: torch.Tensor) -> torch.Tensor:
        """recv [world, *send.shape] in rank order."""
        recv = torch.empty((self.world, *send.shape), dtype=send.dtype, device=send.device)
        self._note_capture()
        _launch("bess_allgather", self.device, self._h, self._buf(send, "send"), self._buf(recv, "recv"),
                send.numel() * send.element_size())
        return recv

    def all_reduce_sum_(self, x: torch.Tensor) -> torch.Tensor:
        """In-place sum over ranks of a float32 tensor."""
        _f32(x, "x")
        self._note_capture()
        p = self._buf(x, "x")
        _launch("bess_allreduce_sum_f32", self.device, self._h, p, p, x.numel())
        return x

    def pack_exchange(self, table: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """K1 + C1: idx [world, L] rows of `table` -> (send, recv), both [world, L, W]."""
        W = int(table.shape[1])
        _rows(table, "table", W)
        if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != self.world or not idx.is_contiguous():
            raise ValueError("pack_exchange: idx must be a contiguous int32 [world, L] tensor")
        L = int(idx.shape[1])
        send = torch.empty((self.world, L, W), dtype=table.dtype, device=table.device)
        recv = torch.empty_like(send)
        self._note_capture()
        _launch("bess_pack_exchange", self.device, self._h, _dtype_code(table), W, self._buf(table, "table"),
                self._buf(idx, "idx"), L, send.data_ptr(), recv.data_ptr())
        return send, recv


# --------------------------------------------------------------------------- #
# recorded steps
GRAPH_NODE_KINDS = ("kernel", "memcpy", "memset", "host", "graph", "empty", "wait_event", "event_record",
                    "ext_sem_signal", "ext_sem_wait", "mem_alloc", "mem_free", "memcpy_from_symbol",
                    "memcpy_to_symbol", "batch_mem_op")


def graph_node_counts(graph: Any) -> dict:
    """Node types of a recorded step: `graph` is a `torch.cuda.CUDAGraph(keep_graph=True)` (its hipGraph_t is
    `raw_cuda_graph()`) or a raw `hipGraph_t` address.  {"kernel": n, "memset": n, ...}, zero counts left out."""
    raw = graph if isinstance(graph, int) else graph.raw_cuda_graph()
    counts = (ctypes.c_int32 * len(GRAPH_NODE_KINDS))()
    _check(load().bess_graph_node_counts(ctypes.c_void_p(raw), counts, len(GRAPH_NODE_KINDS)),
           "bess_graph_node_counts")
    return {k: int(c) for k, c in zip(GRAPH_NODE_KINDS, counts) if c}


# --------------------------------------------------------------------------- #
# step plans (csrc/plan.hip): a step as a recorded list of the library's own calls, replayed from C
PLAN_ARG_INT, PLAN_ARG_FLOAT, PLAN_ARG_PTR, PLAN_ARG_BLOB, PLAN_ARG_STREAM = 0, 1, 2, 3, 4
_INT_TYPES = (ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int)


class Plan:
    """`bess_plan*`: the calls of one recorded step (`record_plan`); `run()` issues them again on PyTorch's current
    stream of `device` - no Python between the calls, and none of the GIL while they are issued (ctypes releases it
    for the duration of a foreign call), so a process that drives several GPUs runs one plan per device from one
    host thread each.  The plan names device buffers by address: the recorder's caller keeps them alive and in place
    (`Runner`: a private memory pool + static input buffers)."""

    def __init__(self, device: torch.device) -> None:
        self.device = device
        self._h = _vp()
        _check(load().bess_plan_create(ctypes.byref(self._h)), "bess_plan_create")
        self.names: List[str] = []

    def __len__(self) -> int:
        return int(load().bess_plan_length(self._h))

    def _add(self, name: str, args: Sequence[Any]) -> None:
        """Note a call of entry point `name` (`_launch`): `args` are all its arguments but the trailing stream, which
        a replay supplies."""
        n = len(args) + 1
        kinds = (ctypes.c_uint8 * n)()
        values = (ctypes.c_uint64 * n)()
        blobs = (_vp * n)()
        sizes = (_i64 * n)()
        keep = []  # the ctypes objects whose bytes are copied must outlive the call
        kinds[n - 1] = PLAN_ARG_STREAM
        for k, (tp, a) in enumerate(zip(SIGNATURES[name], args)):
            if tp in _INT_TYPES:
                kinds[k], values[k] = PLAN_ARG_INT, int(a) & 0xFFFFFFFFFFFFFFFF
            elif tp is ctypes.c_float or tp is ctypes.c_double:
                kinds[k] = PLAN_ARG_FLOAT
                values[k] = ctypes.c_uint64.from_buffer_copy(ctypes.c_double(float(a))).value
            elif tp is _vp:
                kinds[k] = PLAN_ARG_PTR
                values[k] = int(a.value or 0) if isinstance(a, ctypes.c_void_p) else int(a or 0)
            else:  # POINTER(...): NULL, byref(struct), or a ctypes array - host bytes the call reads
                obj = getattr(a, "_obj", a)
                if a is None:
                    kinds[k], values[k] = PLAN_ARG_PTR, 0
                elif isinstance(obj, (ctypes.Structure, ctypes.Array, ctypes._SimpleCData)):
                    kinds[k] = PLAN_ARG_BLOB
                    blobs[k], sizes[k] = ctypes.addressof(obj), ctypes.sizeof(obj)
                    keep.append(obj)
                else:
                    raise TypeError(f"record_plan: {name} argument {k}: cannot record a {type(a).__name__}")
        _check(load().bess_plan_add_call(self._h, name.encode(), n, kinds, values, blobs, sizes), "bess_plan_add_call")
        self.names.append(name)

    def run(self) -> None:
        with _on(self.device):
            rc = load().bess_plan_run(self._h, _stream(self.device))
        _check(rc, "bess_plan_run")

    def run_on(self, stream: int) -> None:
        """`bess_plan_run` on a raw hipStream_t (worker threads of a multi-device process: the device must be the
        thread's current one)."""
        _check(load().bess_plan_run(self._h, stream), "bess_plan_run")

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            h, self._h = self._h, _vp()
            load().bess_plan_destroy(h)

    def __del__(self, _finalizing: Any = sys.is_finalizing) -> None:  # pragma: no cover
        if not _finalizing():
            try:
                self.close()
            except Exception:
                pass


@contextlib.contextmanager
def record_plan(device: torch.device):
    """Run a step inside this context: it executes as usual, and every library call that the calling host thread
    puts on a stream (`_launch`) is noted in the `Plan` the context yields (`plan.run()` issues them again).  Other
    threads' calls are not, so threads that drive different devices record their plans at the same time.  The step
    must be made of library calls only - work enqueued by anything else (a torch operator) is not part of the plan -
    and must not allocate device memory outside a pool the caller keeps (see `Runner._call_with_plans`)."""
    if _recording.plan is not None:
        raise RuntimeError("record_plan: already recording")
    plan = _recording.plan = Plan(device)
    try:
        yield plan
    finally:
        _recording.plan = None
