"""ctypes binding of include/bppp.h.  Data crosses as numpy uint64 arrays (4 limbs per scalar,
8 per affine point, little-endian) or as raw device pointers (ints, e.g. torch.Tensor.data_ptr())."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
NUM_STAGES = 6
STAGE_NAMES = ["digits", "sort", "acc_points", "acc_records", "reduce", "finish"]

# every symbol include/bppp.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "bppp_ctx_create", "bppp_ctx_destroy", "bppp_ctx_set_stream", "bppp_last_error", "bppp_version",
    "bppp_msm", "bppp_msm_device", "bppp_msm_batch_device", "bppp_sum_points", "bppp_rational_reduce",
    "bppp_fold_points", "bppp_fold_points_device", "bppp_rational_reduce_eis", "bppp_fold_points_eis_device",
    "bppp_norm_round_sums_device", "bppp_lin_round_sums_device",
    "bppp_norm_round_openings_device", "bppp_lin_round_openings_device",
    "bppp_fold_scalars_device", "bppp_tensor_device", "bppp_batch_inverse_device",
    "bppp_nl_create", "bppp_nl_destroy", "bppp_nl_lengths", "bppp_nl_round_commit", "bppp_nl_round_collapse",
    "bppp_nl_get_witness", "bppp_nl_download", "bppp_nl_verify", "bppp_nl_verify_batch_device", "bppp_nl_prove", "bppp_nl_verify_challenges",
    "bppp_nlb_create", "bppp_nlb_destroy", "bppp_nlb_lengths", "bppp_nlb_round_commit", "bppp_nlb_round_collapse", "bppp_nlb_get_witness",
    "bppp_ip_create", "bppp_ip_destroy", "bppp_ip_lengths", "bppp_ip_round_commit", "bppp_ip_round_collapse", "bppp_ip_get_witness", "bppp_ip_verify", "bppp_ip_verify_batch_device",
    "bppp_lift_x_device", "bppp_device_alloc", "bppp_device_free", "bppp_upload", "bppp_download", "bppp_host_alloc", "bppp_host_free",
    "bppp_profile_enable", "bppp_profile_read",
    "bppp_trrp_create", "bppp_trrp_destroy", "bppp_trrp_public_device",
    "bppp_glv_decompose_device", "bppp_msm_glv_device",
    "bppp_basis_create", "bppp_basis_create_device", "bppp_basis_destroy", "bppp_basis_info", "bppp_msm_basis", "bppp_basis_enable_comb",
    "bppp_rp_create", "bppp_rp_create_binary", "bppp_rp_destroy", "bppp_rp_info", "bppp_rp_set_option", "bppp_rp_shape_of", "bppp_rp_digits", "bppp_hash_to_scalar", "bppp_rp_verify_batch", "bppp_rp_verify_batch_device", "bppp_rp_verify_shard_device", "bppp_rp_prove_batch",
    "bppp_rp_verify_mixed", "bppp_rp_verify_mixed_device", "bppp_rp_verify_each", "bppp_rp_verify_each_device",
    "bppp_rp_public_count", "bppp_rp_verify_batch_pub", "bppp_rp_verify_batch_pub_device", "bppp_rp_verify_shard_pub_device", "bppp_rp_verify_each_pub",
    "bppp_rp_verify_each_pub_device", "bppp_rp_prove_batch_pub",
    "bppp_rp_share_comb", "bppp_rp_comb_info", "bppp_rp_prove_mixed",
    "bppp_rp_prove_batch_device",
    "bppp_rp_prove_batch_status", "bppp_rp_prove_batch_status_device", "bppp_rp_witness_status_text",
    "bppp_rp_verify_bound", "bppp_rp_verify_bound_device", "bppp_rp_verify_each_bound", "bppp_rp_verify_each_bound_device", "bppp_rp_prove_bound", "bppp_rp_prove_bound_device",
    "bppp_rp_commit_batch", "bppp_rp_commit_batch_device", "bppp_rp_open_each", "bppp_rp_open_each_device", "bppp_rp_open_batch", "bppp_rp_open_batch_device",
    "bppp_rp_tally_each", "bppp_rp_tally_each_device", "bppp_rp_tally_batch", "bppp_rp_tally_batch_device", "bppp_rp_tally_claims", "bppp_rp_tally_claims_device",
    "bppp_rp_excess_sign", "bppp_rp_excess_sign_device", "bppp_rp_excess_verify_each", "bppp_rp_excess_verify_each_device", "bppp_rp_excess_verify_batch",
    "bppp_rp_excess_verify_batch_device",
    "bppp_rp_excess_keys", "bppp_rp_excess_keys_device", "bppp_rp_excess_verify_keys_each", "bppp_rp_excess_verify_keys_each_device", "bppp_rp_excess_verify_keys_batch",
    "bppp_rp_excess_verify_keys_batch_device", "bppp_rp_excess_sums_each", "bppp_rp_excess_sums_each_device", "bppp_rp_excess_sums_batch", "bppp_rp_excess_sums_batch_device",
    "bppp_rp_excess_part_nonces", "bppp_rp_excess_part_nonces_device", "bppp_rp_excess_part_aggregate", "bppp_rp_excess_part_aggregate_device", "bppp_rp_excess_part_sign",
    "bppp_rp_excess_part_sign_device", "bppp_rp_excess_part_verify", "bppp_rp_excess_part_verify_device", "bppp_rp_excess_part_combine", "bppp_rp_excess_part_combine_device",
    "bppp_seed_candidate_x", "bppp_points_from_seed", "bppp_points_from_seed_device", "bppp_rp_create_seeded", "bppp_rp_create_binary_seeded",
    "bppp_rp_verify_block", "bppp_rp_verify_block_device",
    "bppp_rp_excess_halfagg", "bppp_rp_excess_halfagg_device", "bppp_rp_excess_halfagg_verify", "bppp_rp_excess_halfagg_verify_device",
    "bppp_rp_verify_block_agg", "bppp_rp_verify_block_agg_device",
    "bppp_rp_seal", "bppp_rp_seal_device", "bppp_rp_scan", "bppp_rp_scan_device",
    "bppp_rp_scan_keys", "bppp_rp_scan_keys_device",
    "bppp_rp_cut_through", "bppp_rp_cut_through_device",
    "bppp_rp_set_create", "bppp_rp_set_restore", "bppp_rp_set_destroy", "bppp_rp_set_append", "bppp_rp_set_info", "bppp_rp_set_root", "bppp_rp_set_peaks",
    "bppp_rp_set_path_bytes", "bppp_rp_set_paths", "bppp_rp_set_verify_paths",
]


class RpBlock(C.Structure):
    """bppp_rp_block (include/bppp.h): host pointers for bppp_rp_verify_block, HBM pointers for bppp_rp_verify_block_device"""
    _fields_ = [("rows", C.c_size_t), ("coms_files", C.c_void_p), ("nproofs", C.c_size_t), ("proof_files", C.c_void_p), ("bindings", C.c_void_p),
                ("nsums", C.c_size_t), ("sum_start", C.c_void_p), ("entries", C.c_void_p), ("nnz", C.c_size_t),
                ("claim_amounts", C.c_void_p), ("claim_types", C.c_void_p), ("claim_offsets", C.c_void_p),
                ("nkeys", C.c_size_t), ("key_start", C.c_void_p), ("keys", C.c_void_p), ("msgs", C.c_void_p), ("sigs", C.c_void_p),
                ("proof_offset", C.c_uint64), ("key_offset", C.c_uint64), ("sum_offset", C.c_uint64)]


class RpCutCounts(C.Structure):
    """bppp_rp_cut_counts: what bppp_rp_cut_through left — rows of the new pool, how many of them are new outputs, surviving entries, entries cut, entries kept again"""
    _fields_ = [(n, C.c_size_t) for n in ("new_rows", "out_rows", "new_nnz", "ncut", "nagain")]


class RpBlockStatus(C.Structure):
    """bppp_rp_block_status: three host arrays of uint32, each may be NULL"""
    _fields_ = [("proof_status", C.c_void_p), ("key_status", C.c_void_p), ("sum_status", C.c_void_p)]


class BpppError(RuntimeError):
    pass


def lib_path() -> str:
    return os.path.join(_HERE, "lib", "libbppp_hip.so")


def load_library() -> C.CDLL:
    p = lib_path()
    if not os.path.exists(p):
        raise BpppError(f"{p} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(p)
    u64p, vp, sz, i = C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t, C.c_int
    lib.bppp_ctx_create.argtypes = [i, C.POINTER(vp)]
    lib.bppp_ctx_destroy.argtypes = [vp]
    lib.bppp_ctx_destroy.restype = None
    lib.bppp_ctx_set_stream.argtypes = [vp, vp]
    lib.bppp_last_error.argtypes = [vp]
    lib.bppp_last_error.restype = C.c_char_p
    lib.bppp_version.restype = C.c_char_p
    lib.bppp_msm.argtypes = [vp, vp, vp, sz, vp]
    lib.bppp_msm_device.argtypes = [vp, vp, vp, sz, i, vp]
    lib.bppp_msm_batch_device.argtypes = [vp, vp, vp, sz, sz, i, i, vp]
    lib.bppp_sum_points.argtypes = [vp, vp, sz, vp]
    lib.bppp_glv_decompose_device.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.bppp_msm_glv_device.argtypes = [vp, vp, vp, sz, vp]
    lib.bppp_rational_reduce.argtypes = [vp, vp, C.POINTER(i), vp, C.POINTER(i)]
    lib.bppp_rational_reduce_eis.argtypes = [vp, vp, vp, vp, vp]
    lib.bppp_fold_points_eis_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp]
    lib.bppp_fold_points.argtypes = [vp, vp, i, vp, i, vp, sz, vp]
    lib.bppp_fold_points_device.argtypes = [vp, vp, i, vp, i, vp, sz, vp]
    lib.bppp_norm_round_sums_device.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.bppp_lin_round_sums_device.argtypes = [vp, vp, vp, sz, vp, vp]
    lib.bppp_norm_round_openings_device.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    lib.bppp_lin_round_openings_device.argtypes = [vp, vp, sz, vp, vp]
    lib.bppp_fold_scalars_device.argtypes = [vp, vp, vp, vp, sz, vp]
    lib.bppp_batch_inverse_device.argtypes = [vp, vp, sz, i, vp]
    lib.bppp_tensor_device.argtypes = [vp, vp, sz, vp, vp, sz, vp]
    lib.bppp_lift_x_device.argtypes = [vp, vp, sz, vp]
    lib.bppp_trrp_create.argtypes = [vp, i, i, sz, sz, sz, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, C.POINTER(vp)]
    lib.bppp_trrp_destroy.argtypes = [vp]
    lib.bppp_trrp_destroy.restype = None
    lib.bppp_trrp_public_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    lib.bppp_nl_create.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, C.POINTER(vp)]
    lib.bppp_nl_destroy.argtypes = [vp]
    lib.bppp_nl_destroy.restype = None
    lib.bppp_nl_lengths.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    lib.bppp_nl_round_commit.argtypes = [vp, vp, vp, vp, vp]
    lib.bppp_nl_round_collapse.argtypes = [vp, vp]
    lib.bppp_nl_get_witness.argtypes = [vp, vp, vp]
    lib.bppp_nl_download.argtypes = [vp] + [vp] * 9
    lib.bppp_nl_prove.argtypes = [vp, sz, vp, vp, vp, C.POINTER(sz), sz, vp, vp]
    lib.bppp_nl_verify_challenges.argtypes = [vp, vp, vp, sz, vp, C.POINTER(sz), sz, vp]
    lib.bppp_nlb_create.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, C.POINTER(vp)]
    lib.bppp_nlb_destroy.argtypes = [vp]
    lib.bppp_nlb_destroy.restype = None
    lib.bppp_nlb_lengths.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    lib.bppp_nlb_round_commit.argtypes = [vp, vp, vp, vp, vp]
    lib.bppp_nlb_round_collapse.argtypes = [vp, vp]
    lib.bppp_nlb_get_witness.argtypes = [vp, vp, vp, vp]
    lib.bppp_ip_create.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, C.POINTER(vp)]
    lib.bppp_ip_destroy.argtypes = [vp]
    lib.bppp_ip_destroy.restype = None
    lib.bppp_ip_lengths.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    lib.bppp_ip_round_commit.argtypes = [vp, vp, vp, vp, vp]
    lib.bppp_ip_round_collapse.argtypes = [vp, vp]
    lib.bppp_ip_get_witness.argtypes = [vp, vp, vp, vp]
    lib.bppp_ip_verify.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp, sz, vp, sz, vp, sz, vp, vp, sz, vp, vp]
    lib.bppp_nl_verify_batch_device.argtypes = [vp] + [sz] * 7 + [vp] * 16
    lib.bppp_ip_verify_batch_device.argtypes = [vp] + [sz] * 7 + [vp] * 16
    lib.bppp_nl_verify.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp, sz, vp, sz, vp, sz, vp, vp, sz, vp, vp]
    lib.bppp_device_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    lib.bppp_device_free.argtypes = [vp, vp]
    lib.bppp_host_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    lib.bppp_host_free.argtypes = [vp, vp]
    lib.bppp_upload.argtypes = [vp, vp, vp, sz]
    lib.bppp_download.argtypes = [vp, vp, vp, sz]
    lib.bppp_basis_create.argtypes = [vp, vp, sz, i, sz, C.POINTER(vp)]
    lib.bppp_basis_create_device.argtypes = [vp, vp, sz, i, sz, C.POINTER(vp)]
    lib.bppp_basis_destroy.argtypes = [vp]
    lib.bppp_basis_destroy.restype = None
    lib.bppp_basis_info.argtypes = [vp, C.POINTER(sz), C.POINTER(i), C.POINTER(sz)]
    lib.bppp_msm_basis.argtypes = [vp, vp, sz, sz, vp]
    lib.bppp_basis_enable_comb.argtypes = [vp, C.c_int, sz, vp, vp]
    lib.bppp_rp_create.argtypes = [vp, i, i, vp, sz, vp, sz, vp, sz, C.c_char_p, C.POINTER(vp)]
    lib.bppp_rp_create_binary.argtypes = [vp, i, i, vp, sz, vp, vp, sz, C.c_char_p, C.POINTER(vp)]
    lib.bppp_rp_destroy.argtypes = [vp]
    lib.bppp_rp_destroy.restype = None
    lib.bppp_rp_info.argtypes = [vp, vp]
    lib.bppp_rp_set_option.argtypes = [vp, i, C.c_uint64]
    lib.bppp_rp_shape_of.argtypes = [i, i, vp, sz, vp]
    lib.bppp_rp_digits.argtypes = [vp, vp, vp, sz, C.POINTER(sz), C.POINTER(i)]
    lib.bppp_hash_to_scalar.argtypes = [vp, sz, vp]
    lib.bppp_rp_verify_batch.argtypes = [vp, sz, vp, vp, vp, C.POINTER(i), vp, vp, vp]
    lib.bppp_rp_verify_batch_device.argtypes = [vp, sz, vp, vp, vp, C.POINTER(i), vp, vp, vp]
    lib.bppp_rp_verify_shard_device.argtypes = [vp, sz, C.c_uint64, vp, vp, vp, C.POINTER(i), vp, vp, vp]
    lib.bppp_rp_prove_batch.argtypes = [vp, sz, vp, vp, vp, vp, sz, vp, vp]
    lib.bppp_rp_verify_mixed.argtypes = [vp, sz, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_verify_mixed_device.argtypes = [vp, sz, C.c_uint64, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_verify_each.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.bppp_rp_verify_each_device.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.bppp_rp_public_count.argtypes = [vp, C.POINTER(sz)]
    lib.bppp_rp_verify_batch_pub.argtypes = [vp, sz, vp, vp, vp, vp, C.POINTER(i), vp, vp, vp]
    lib.bppp_rp_verify_batch_pub_device.argtypes = [vp, sz, vp, vp, vp, vp, C.POINTER(i), vp, vp, vp]
    lib.bppp_rp_verify_shard_pub_device.argtypes = [vp, sz, C.c_uint64, vp, vp, vp, vp, C.POINTER(i), vp, vp, vp]
    lib.bppp_rp_verify_each_pub.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_verify_each_pub_device.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_prove_batch_pub.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, vp, vp]
    lib.bppp_rp_share_comb.argtypes = [vp, vp]
    lib.bppp_rp_comb_info.argtypes = [vp, C.POINTER(i), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    lib.bppp_rp_prove_mixed.argtypes = [vp, sz]
    lib.bppp_rp_prove_batch_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, vp, vp]
    lib.bppp_rp_prove_batch_status.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, vp, vp, vp]
    lib.bppp_rp_prove_batch_status_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, vp, vp, vp]
    lib.bppp_rp_witness_status_text.argtypes = [C.c_uint32]
    lib.bppp_rp_witness_status_text.restype = C.c_char_p
    lib.bppp_rp_verify_bound.argtypes = [vp, sz, vp, vp, vp, vp, vp, C.POINTER(i), vp, vp, vp]
    lib.bppp_rp_verify_bound_device.argtypes = [vp, sz, C.c_uint64, vp, vp, vp, vp, vp, C.POINTER(i), vp, vp, vp]
    lib.bppp_rp_verify_each_bound.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_verify_each_bound_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_prove_bound.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]
    lib.bppp_rp_prove_bound_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]
    lib.bppp_rp_commit_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_commit_batch_device.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_open_each.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_open_each_device.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_open_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_open_batch_device.argtypes = [vp, sz, C.c_uint64, vp, vp, vp, vp, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_tally_each.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_tally_each_device.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_tally_batch.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_tally_batch_device.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, C.c_uint64, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_tally_claims.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, sz, vp, vp, vp]
    lib.bppp_rp_tally_claims_device.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, sz, vp, vp, vp]
    lib.bppp_rp_excess_sign.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_sign_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_verify_each.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_verify_each_device.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_verify_batch.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_excess_verify_batch_device.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp, C.c_uint64, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_excess_keys.argtypes = [vp, sz, vp, vp, vp]
    lib.bppp_rp_excess_keys_device.argtypes = [vp, sz, vp, vp, vp]
    lib.bppp_rp_excess_verify_keys_each.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.bppp_rp_excess_verify_keys_each_device.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.bppp_rp_excess_verify_keys_batch.argtypes = [vp, sz, vp, vp, vp, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_excess_verify_keys_batch_device.argtypes = [vp, sz, vp, vp, vp, C.c_uint64, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_excess_sums_each.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.bppp_rp_excess_sums_each_device.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.bppp_rp_excess_sums_batch.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_excess_sums_batch_device.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, sz, vp, vp, C.c_uint64, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_excess_part_nonces.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_part_nonces_device.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_part_aggregate.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_part_aggregate_device.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_part_sign.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_part_sign_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_part_verify.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_part_verify_device.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_part_combine.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_part_combine_device.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_verify_block.argtypes = [vp, C.POINTER(RpBlock), vp, C.POINTER(i), C.POINTER(RpBlockStatus), vp]
    lib.bppp_rp_verify_block_device.argtypes = [vp, C.POINTER(RpBlock), vp, C.POINTER(i), C.POINTER(RpBlockStatus), vp]
    lib.bppp_rp_excess_halfagg.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_halfagg_device.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_rp_excess_halfagg_verify.argtypes = [vp, sz, vp, vp, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_excess_halfagg_verify_device.argtypes = [vp, sz, vp, vp, vp, C.POINTER(i), vp, vp]
    lib.bppp_rp_verify_block_agg.argtypes = [vp, C.POINTER(RpBlock), vp, vp, C.POINTER(i), C.POINTER(RpBlockStatus), vp]
    lib.bppp_rp_verify_block_agg_device.argtypes = [vp, C.POINTER(RpBlock), vp, vp, C.POINTER(i), C.POINTER(RpBlockStatus), vp]
    lib.bppp_rp_seal.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_seal_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.bppp_rp_scan.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(sz)]
    lib.bppp_rp_scan_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(sz)]
    lib.bppp_rp_scan_keys.argtypes = [vp, sz, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp, C.POINTER(sz), C.POINTER(C.c_uint64)]
    lib.bppp_rp_scan_keys_device.argtypes = [vp, sz, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp, C.POINTER(sz), C.POINTER(C.c_uint64)]
    lib.bppp_rp_cut_through.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(RpCutCounts)]
    lib.bppp_rp_cut_through_device.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(RpCutCounts)]
    lib.bppp_rp_set_create.argtypes = [vp, sz, i, C.POINTER(vp)]
    lib.bppp_rp_set_restore.argtypes = [vp, sz, C.c_uint64, vp, C.POINTER(vp)]
    lib.bppp_rp_set_destroy.argtypes = [vp]
    lib.bppp_rp_set_destroy.restype = None
    lib.bppp_rp_set_append.argtypes = [vp, sz, vp]
    lib.bppp_rp_set_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    lib.bppp_rp_set_root.argtypes = [vp, vp]
    lib.bppp_rp_set_peaks.argtypes = [vp, vp]
    lib.bppp_rp_set_path_bytes.argtypes = [C.c_uint64]
    lib.bppp_rp_set_path_bytes.restype = sz
    lib.bppp_rp_set_paths.argtypes = [vp, sz, vp, vp]
    lib.bppp_rp_set_verify_paths.argtypes = [vp, sz, C.c_uint64, vp, sz, vp, vp, vp, vp, C.POINTER(C.c_int)]
    lib.bppp_seed_candidate_x.argtypes =[C.c_char_p, sz, C.c_uint64, vp]
    lib.bppp_points_from_seed.argtypes = [vp, C.c_char_p, sz, C.c_uint64, sz, vp, C.POINTER(C.c_uint64)]
    lib.bppp_points_from_seed_device.argtypes = [vp, C.c_char_p, sz, C.c_uint64, sz, vp, C.POINTER(C.c_uint64)]
    lib.bppp_rp_create_seeded.argtypes = [vp, i, i, vp, sz, vp, sz, C.c_char_p, sz, C.c_char_p, C.POINTER(vp)]
    lib.bppp_rp_create_binary_seeded.argtypes = [vp, i, i, vp, sz, vp, C.c_char_p, sz, C.c_char_p, C.POINTER(vp)]
    lib.bppp_profile_enable.argtypes = [vp, i]
    lib.bppp_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), i]
    return lib


def load_test_library() -> C.CDLL:
    """libbppp_hip_test.so: the bppp_test_* hooks of include/bppp_test.h (parity tests, bench.py's multiply-rate probe).
    They take the product library's context handle; nothing in the product depends on them."""
    p = os.path.join(_HERE, "lib", "libbppp_hip_test.so")
    if not os.path.exists(p):
        raise BpppError(f"{p} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(p)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    lib.bppp_test_fe_op.argtypes = [vp, i, i, vp, vp, sz, vp]
    lib.bppp_test_point_op.argtypes = [vp, i, vp, vp, sz, vp]
    lib.bppp_test_point_quad.argtypes = [vp, i, vp, vp, sz, vp, vp]
    lib.bppp_test_fq_pair.argtypes = [vp, i, vp, vp, vp, vp, sz, vp]
    lib.bppp_test_point_chain.argtypes = [vp, i, vp, vp, sz, vp, vp]
    lib.bppp_test_mulmod_rate.argtypes = [vp, i, C.POINTER(C.c_double)]
    lib.bppp_test_last_mixed_msm_terms.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.bppp_test_last_sort_ranges.argtypes = [vp, C.POINTER(C.c_int)]
    lib.bppp_test_last_scatter_one_read.argtypes = [vp, C.POINTER(C.c_int)]
    lib.bppp_test_last_hist16.argtypes = [vp, C.POINTER(C.c_int)]
    lib.bppp_test_last_acc_sized.argtypes = [vp, C.POINTER(C.c_int)]
    lib.bppp_test_last_acc_fq29.argtypes = [vp, C.POINTER(C.c_int)]
    lib.bppp_test_fq29_op.argtypes = [vp, i, vp, vp, sz, vp, vp]
    lib.bppp_test_madd29_chain.argtypes = [vp, vp, vp, sz, sz, vp, vp]
    lib.bppp_test_madd26_chain.argtypes = [vp, vp, vp, sz, sz, vp, vp]
    lib.bppp_test_ec29_fast_op.argtypes = [vp, i, vp, sz, vp]
    lib.bppp_test_last_msm_layout.argtypes = [vp, C.POINTER(TestMsmLayout)]
    lib.bppp_test_last_msm_copy.argtypes = [vp, i, vp, sz]
    lib.bppp_test_last_windows.argtypes = [vp, C.POINTER(C.c_int)]
    lib.bppp_test_rp_last_verify_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.bppp_test_rp_last_block_counts.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
    lib.bppp_test_rp_set_each_chunk.argtypes = [vp, sz]
    lib.bppp_test_rp_set_tally_short_max.argtypes = [vp, sz]
    lib.bppp_test_rp_set_tally_piece.argtypes = [vp, sz]
    lib.bppp_test_rp_set_tally_chunk.argtypes = [vp, sz]
    lib.bppp_test_rp_set_flat_chunk.argtypes = [vp, sz]
    lib.bppp_test_rp_excess_mul.argtypes = [vp, sz, vp, vp, vp]
    lib.bppp_test_rp_excess_mul2.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.bppp_test_rp_scan_mul.argtypes = [vp, sz, vp, vp, vp]
    lib.bppp_test_rp_scan_recode.argtypes = [vp, vp]
    lib.bppp_test_rp_scan_keys_mul.argtypes = [vp, sz, vp, sz, vp, vp]
    lib.bppp_test_rp_scan_keys_recode.argtypes = [vp, vp]
    lib.bppp_test_rp_scan_keys_geometry.argtypes = [vp, sz, sz, vp]
    lib.bppp_test_rp_witness_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.bppp_test_points_from_seed_chunked.argtypes = [vp, C.c_char_p, sz, C.c_uint64, sz, sz, vp, C.POINTER(C.c_uint64)]
    lib.bppp_test_seed_lift_digests.argtypes = [vp, C.c_char_p, sz, vp, vp, vp]
    lib.bppp_test_rp_decode_device.argtypes = [vp, sz, C.c_char_p, C.c_char_p, vp, vp, vp, vp, vp, vp]
    lib.bppp_test_comb_create.argtypes = [vp, vp, sz, i, C.POINTER(vp)]
    lib.bppp_test_comb_destroy.argtypes = [vp]
    lib.bppp_test_comb_destroy.restype = None
    lib.bppp_test_comb_msm.argtypes = [vp, vp, sz, sz, i, sz, vp]
    lib.bppp_test_comb_groups.argtypes = [vp, vp, sz, sz, sz, i, sz, vp]
    lib.bppp_test_comb_lanes.argtypes = [vp, vp, sz, sz, vp]
    lib.bppp_test_last_comb_msm.argtypes = [vp, C.POINTER(TestCombReport)]
    lib.bppp_test_last_reduce.argtypes = [vp, C.POINTER(TestReduceReport)]
    lib.bppp_test_rp_last_text_kernel.argtypes = [vp, C.POINTER(C.c_int)]
    lib.bppp_test_rp_lds_plan.argtypes = [i, sz, sz, sz, sz, C.POINTER(TestRpLdsPlan)]
    lib.bppp_test_rp_last_prove.argtypes = [vp, C.POINTER(TestRpProveReport)]
    lib.bppp_test_trrp_last_public.argtypes = [vp, C.POINTER(TestRpPublicReport)]
    lib.bppp_test_rp_last_public.argtypes = [vp, C.POINTER(TestRpPublicReport)]
    lib.bppp_test_rpp_transcript.argtypes = [vp, sz, vp, sz, vp, vp, vp]
    lib.bppp_test_rpp_draws.argtypes = [vp, C.c_char_p, sz, sz, sz, vp]
    lib.bppp_test_ctx_poison.argtypes = [vp, i, C.POINTER(C.c_uint64)]
    lib.bppp_test_rp_poison.argtypes = [vp, i, C.POINTER(C.c_uint64)]
    lib.bppp_test_rp_cut_through_force.argtypes = [vp, i, vp, i]
    lib.bppp_test_rp_cut_through_last.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 3
    return lib


class TestCombReport(C.Structure):
    """bppp_test_comb_report (include/bppp_test.h): what the last comb_msm launch on a context did"""
    __test__ = False                      # not a pytest class
    _fields_ = [("route", C.c_int32), ("heavy_first", C.c_int32)] + [(n, C.c_uint32) for n in ("parts", "tparts", "wsplit", "chunks", "clen", "join_lanes")]


class TestRpLdsPlan(C.Structure):
    """bppp_test_rp_lds_plan_report (include/bppp_test.h): the planned dynamic LDS of one of the size-dependent typed-reciprocal kernels"""
    __test__ = False
    _fields_ = [("lds_bytes", C.c_uint64)] + [(n, C.c_uint32) for n in ("table", "lanes", "fits", "split")]


class TestRpProveReport(C.Structure):
    """bppp_test_rp_prove_report: what the last typed-reciprocal prove on a handle ran"""
    __test__ = False
    _fields_ = [("route", C.c_int32), ("table", C.c_uint32), ("lds2_bytes", C.c_uint64), ("lds3_bytes", C.c_uint64)]


class TestRpPublicReport(C.Structure):
    """bppp_test_rp_public_report: what the last bppp_trrp_public_device on a setup's tables launched"""
    __test__ = False
    _fields_ = [("route", C.c_int32), ("lanes", C.c_int32), ("lds_bytes", C.c_uint64)]


# bppp_test_rp_lds_plan's kernels, the routes of bppp_test_rp_last_prove and of bppp_test_*_last_public
TEST_RP_K_PUBLIC, TEST_RP_K_PHASE2, TEST_RP_K_PHASE3 = 0, 2, 3
TEST_RP_PROVE_DEVICE_ALGEBRA, TEST_RP_PROVE_HOST_ALGEBRA = 1, 2
TEST_RP_PUBLIC_ONE_KERNEL, TEST_RP_PUBLIC_THREE_KERNELS = 1, 2


class TestReduceReport(C.Structure):
    """bppp_test_reduce_report (include/bppp_test.h): what the bucket reduction of the last MSM on a context launched"""
    __test__ = False
    _fields_ = [(n, C.c_int32) for n in ("route", "combine", "c", "W", "M", "RG", "Lw", "WPW", "a", "LO", "HI", "PR", "PC", "SR", "SC", "TR", "TC", "S")]


class TestMsmLayout(C.Structure):
    """bppp_test_msm_layout (include/bppp_test.h): the plan of the last general-pipeline MSM on a context"""
    __test__ = False
    _fields_ = [(n, C.c_int32) for n in ("c", "W", "acnt", "top", "M", "flat", "CH", "Q", "one_read", "sized", "fq29", "L", "shared_points", "acc_fast")] + \
               [(n, C.c_uint32) for n in ("stride", "per")] + [(n, C.c_uint64) for n in ("batch", "n", "FB", "G", "total", "table_stride")]


# bppp_test_last_msm_copy's arrays
TEST_MSM_DIGITS, TEST_MSM_NEGMASK, TEST_MSM_COUNT, TEST_MSM_START, TEST_MSM_SORTED, TEST_MSM_BUCKETS_RAW, TEST_MSM_BUCKETS_AFF = range(7)


class TestRppCall(C.Structure):
    """bppp_test_rpp_call (include/bppp_test.h): one oracle call of bppp_test_rpp_transcript"""
    __test__ = False
    _fields_ = [("points", C.c_uint32), ("count", C.c_uint32), ("first_slot", C.c_uint32)]


class RpRange(C.Structure):
    """bppp_rp_range (include/bppp.h)"""
    _fields_ = [("base", C.c_uint32), ("flags", C.c_uint32), ("min", C.c_uint64 * 4), ("max", C.c_uint64 * 4)]


class RpPublic(C.Structure):
    """bppp_rp_public"""
    _fields_ = [("is_output", C.c_uint32), ("reserved", C.c_uint32), ("type", C.c_uint64 * 4), ("amount", C.c_uint64 * 4)]


class RpGroup(C.Structure):
    """bppp_rp_group: one setup's share of a mixed batch"""
    _fields_ = [("rp", C.c_void_p), ("batch", C.c_size_t), ("coms_files", C.c_void_p), ("proof_files", C.c_void_p)]


class RpProveGroup(C.Structure):
    """bppp_rp_prove_group: one setup's share of a mixed prove job"""
    _fields_ = [("rp", C.c_void_p), ("batch", C.c_size_t), ("amounts", C.c_void_p), ("types", C.c_void_p), ("blinds", C.c_void_p),
                ("public_amounts", C.c_void_p), ("rand_prefix", C.c_void_p), ("prefix_len", C.c_size_t), ("coms_files", C.c_void_p),
                ("proof_files", C.c_void_p)]


class RpShape(C.Structure):
    """bppp_rp_shape"""
    _fields_ = [(n, C.c_size_t) for n in ("nranges", "norm_len", "lin_len", "rounds", "final_norm", "final_lin", "coms_bytes", "proof_bytes",
                                          "challenges_per_proof")]


RP_OPTIONS = {"comb_min": 1, "comb_budget": 2, "comb_bits": 3, "split_min": 4, "host_oracle_max": 5, "fold_points": 6, "host_algebra": 7, "timing": 8, "culprits": 9}
RP_SHARED, RP_OUTPUT, RP_ASSUMED = 1, 2, 4
RP_VALID, RP_INVALID, RP_MALFORMED = 0, 1, 2
# BPPP_RP_WIT_*: a proof's verdict from bppp_rp_prove_batch_status{,_device}
RP_WIT_OK, RP_WIT_NOT_CANONICAL, RP_WIT_UNBALANCED, RP_WIT_OUT_OF_RANGE, RP_WIT_BIN_NOT_CANONICAL, RP_WIT_BIN_UNBALANCED = 0, 1, 2, 3, 4, 5
# bppp_rp_commit_batch's own row verdict next to RP_WIT_OK / _NOT_CANONICAL / _BIN_NOT_CANONICAL, and BPPP_RP_OPEN_*: one opening's verdict
RP_COMMIT_INFINITY = 16
RP_OPEN_OK, RP_OPEN_MISMATCH, RP_OPEN_MALFORMED, RP_OPEN_NOT_CANONICAL = 0, 1, 2, 3
# BPPP_RP_EXCESS_*: bppp_rp_excess_sign's verdicts, and the two bppp_rp_excess_verify_* add to RP_OPEN_*
RP_EXCESS_OK, RP_EXCESS_NOT_CANONICAL, RP_EXCESS_ZERO, RP_EXCESS_NONCE = 0, 1, 2, 3
RP_EXCESS_BAD_R, RP_EXCESS_NO_KEY = 4, 5
RP_EXCESS_SIG_BYTES = 65
# the stated keys (bppp_rp_excess_keys / _verify_keys_* / _sums_*): 33 bytes a key, and the verdict of one that does not lift
RP_EXCESS_KEY_BYTES = 33
RP_EXCESS_BAD_KEY = 6
# the multi-party signer (bppp_rp_excess_part_*): 66 bytes a public nonce, 32 a partial response, and its two verdicts: a nonce sum that is
# infinity, and (part_verify) a part whose sum has no aggregate because another part does not lift
RP_EXCESS_PUBNONCE_BYTES = 66
RP_EXCESS_PARTIAL_BYTES = 32
RP_EXCESS_NONCE_INFINITY = 7
RP_EXCESS_NO_AGGREGATE = 8
# sealed outputs (bppp_rp_seal / bppp_rp_scan): a seal's verdicts next to RP_EXCESS_BAD_KEY, a scanned row's verdicts, the bytes of a seal
RP_SEAL_OK, RP_SEAL_NOT_CANONICAL, RP_SEAL_ZERO = 0, 1, 2
RP_SCAN_FOREIGN, RP_SCAN_OWNED, RP_SCAN_BAD_HINT, RP_SCAN_TAG_ONLY = 0, 1, 2, 3
# BPPP_RP_CUT_*: an entry's verdict from bppp_rp_cut_through
RP_CUT_KEPT, RP_CUT_SPENT, RP_CUT_KEPT_AGAIN = 0, 1, 2
# BPPP_RP_SET_*: a membership path's verdict from bppp_rp_set_verify_paths; the longest row of a set
RP_SET_OK, RP_SET_MISMATCH, RP_SET_BAD_INDEX, RP_SET_BAD_PADDING = 0, 1, 2, 3
RP_SET_MAX_ROW_BYTES = 8192
RP_SCAN_MAX_KEYS = 1 << 20                                     # BPPP_RP_SCAN_MAX_KEYS: view secrets of one bppp_rp_scan_keys call


def SEAL_BYTES(nranges: int) -> int:
    """BPPP_RP_SEAL_BYTES"""
    return 34 + 64 * nranges


# BPPP_RP_BINDING_BYTES: one proof's transcript binding of the bppp_rp_*_bound* entry points
RP_BINDING_BYTES = 32


def bindings_array(bindings, batch: int):
    """The `bindings` argument of the bound range-proof calls as a contiguous [batch, 32] uint8 array: a sequence of 32-byte bytes objects or an
    array of that shape.  None stays None (the unbound call).  A wrong length or shape is a ValueError, raised before any library call."""
    if bindings is None:
        return None
    if isinstance(bindings, np.ndarray):
        if bindings.dtype != np.uint8 or bindings.shape != (batch, RP_BINDING_BYTES):
            raise ValueError(f"bindings: expected a uint8 array of shape ({batch}, {RP_BINDING_BYTES}), got {bindings.dtype} {bindings.shape}")
        return np.ascontiguousarray(bindings)
    rows = list(bindings)
    if len(rows) != batch:
        raise ValueError(f"bindings: {len(rows)} bindings for {batch} proofs")
    for k, r in enumerate(rows):
        if not isinstance(r, (bytes, bytearray)) or len(r) != RP_BINDING_BYTES:
            raise ValueError(f"bindings: binding {k} is not {RP_BINDING_BYTES} bytes")
    return np.frombuffer(b"".join(bytes(r) for r in rows), dtype=np.uint8).reshape(batch, RP_BINDING_BYTES).copy()


# ---- integer <-> limb helpers (host-side glue for tests / bench)
def int_to_limbs(x: int, n: int = 4) -> np.ndarray:
    return np.array([(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(n)], dtype=np.uint64)


def limbs_to_int(a) -> int:
    return sum(int(v) << (64 * k) for k, v in enumerate(np.asarray(a).reshape(-1)))


def scalars_to_array(xs: Sequence[int]) -> np.ndarray:
    out = np.zeros((len(xs), 4), dtype=np.uint64)
    for r, x in enumerate(xs):
        out[r] = int_to_limbs(x)
    return out


def points_to_array(ps) -> np.ndarray:
    out = np.zeros((len(ps), 8), dtype=np.uint64)
    for r, p in enumerate(ps):
        if p is not None:
            out[r, :4] = int_to_limbs(p[0])
            out[r, 4:] = int_to_limbs(p[1])
    return out


def array_to_point(a):
    a = np.asarray(a).reshape(8)
    x, y = limbs_to_int(a[:4]), limbs_to_int(a[4:])
    return None if x == 0 and y == 0 else (x, y)


def array_to_scalars(a):
    a = np.asarray(a).reshape(-1, 4)
    return [limbs_to_int(r) for r in a]


class _Ptr(C.c_void_p):
    """c_void_p that keeps the numpy array it points into alive until the foreign call returns."""
    _keep = None


def _ptr(a) -> C.c_void_p:
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"] and a.dtype in (np.uint64, np.uint32)
        p = _Ptr(a.ctypes.data)
        p._keep = a
        return p
    return C.c_void_p(int(a))  # raw device pointer


class Bppp:
    """One context = one GPU + one HIP stream (include/bppp.h)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.bppp_ctx_create(device, C.byref(h))
        if rc != 0:
            raise BpppError(f"bppp_ctx_create(device={device}) failed with {rc} "
                            "(-3 = no GPU visible; this library has no CPU path)")
        self.h = h
        import weakref
        self._children = weakref.WeakSet()      # child handles (NormLinearBP, ...): closed before the context
        if stream is not None:
            self.set_stream(stream)

    def _adopt(self, child):
        self._children.add(child)

    def close(self):
        """Closes the child handles first, then the context.  (The C ABI is safe in either order — a child keeps its context
        alive until it is destroyed itself — this just releases the device memory promptly.)"""
        if getattr(self, "h", None):
            for ch in list(getattr(self, "_children", ())):
                try:
                    ch.close()
                except Exception:
                    pass
            self.lib.bppp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise BpppError(f"{what} failed ({rc}): {self.lib.bppp_last_error(self.h).decode()}")

    def set_stream(self, stream: int):
        self._check(self.lib.bppp_ctx_set_stream(self.h, C.c_void_p(stream)), "bppp_ctx_set_stream")

    # ---- MSM
    def msm(self, scalars: np.ndarray, points: np.ndarray):
        n = scalars.shape[0] if scalars.size else 0
        out = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.bppp_msm(self.h, _ptr(np.ascontiguousarray(scalars)), _ptr(np.ascontiguousarray(points)), n, _ptr(out)), "bppp_msm")
        return array_to_point(out)

    def msm_device(self, d_scalars: int, d_points: int, n: int, window_bits: int = 0):
        out = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.bppp_msm_device(self.h, _ptr(d_scalars), _ptr(d_points), n, window_bits, _ptr(out)), "bppp_msm_device")
        return array_to_point(out)

    def msm_batch_device(self, d_scalars: int, d_points: int, n: int, batch: int, shared_points: bool, window_bits: int = 0):
        out = np.zeros((batch, 8), dtype=np.uint64)
        self._check(self.lib.bppp_msm_batch_device(self.h, _ptr(d_scalars), _ptr(d_points), n, batch, int(shared_points), window_bits, _ptr(out)),
                    "bppp_msm_batch_device")
        return [array_to_point(out[b]) for b in range(batch)]

    def basis(self, points, window_bits: int = 0, batch_hint: int = 1, device: bool = False, n: int = 0) -> "Basis":
        """register a basis: `points` is an (n, 8) uint64 array, or a device pointer with device=True and n given"""
        return Basis(self, points, window_bits, batch_hint, device, n)

    def msm_glv_device(self, d_scalars: int, d_points: int, n: int):
        """the MSM through the reference's endomorphism decomposition (same group element as msm_device)"""
        out = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.bppp_msm_glv_device(self.h, _ptr(d_scalars), _ptr(d_points), n, _ptr(out)), "bppp_msm_glv_device")
        return array_to_point(out)

    def glv_decompose(self, scalars):
        """decomposeFastPrimeEis for a list of scalars: [(a, b)] as signed Python integers"""
        n = len(scalars)
        d_s = self.to_device(scalars_to_array([s for s in scalars]))
        d_a, d_b, d_g = self.alloc(max(n, 1) * 32), self.alloc(max(n, 1) * 32), self.alloc(max(n, 1) * 4 + 16)
        try:
            self._check(self.lib.bppp_glv_decompose_device(self.h, _ptr(d_s), n, _ptr(d_a), _ptr(d_b), _ptr(d_g)), "bppp_glv_decompose_device")
            a, b = array_to_scalars(self.download(d_a, (n, 4))), array_to_scalars(self.download(d_b, (n, 4)))
            g = self.download(d_g, (n,), dtype=np.uint32)
        finally:
            for p_ in (d_s, d_a, d_b, d_g):
                self.free(p_)
        assert not any(int(x) & 4 for x in g)
        return [(-x if int(f) & 1 else x, -y if int(f) & 2 else y) for x, y, f in zip(a, b, g)]

    def sum_points(self, points: np.ndarray):
        """sum of a few affine points ((n, 8) uint64): the combine step after the all-gather of a sharded MSM"""
        pts = np.ascontiguousarray(points)
        out = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.bppp_sum_points(self.h, _ptr(pts), pts.shape[0] if pts.size else 0, _ptr(out)), "bppp_sum_points")
        return array_to_point(out)

    # ---- reduced scalars / folds
    def rational_reduce(self, x: int) -> Tuple[int, int]:
        am, bm = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
        an, bn = C.c_int(0), C.c_int(0)
        rc = self.lib.bppp_rational_reduce(_ptr(int_to_limbs(x)), _ptr(am), C.byref(an), _ptr(bm), C.byref(bn))
        if rc != 0:
            raise BpppError(f"bppp_rational_reduce failed ({rc})")
        a, b = limbs_to_int(am), limbs_to_int(bm)
        return (-a if an.value else a, -b if bn.value else b)

    def rational_reduce_eis(self, x: int):
        """((a0, a1), (b0, b1)): the Eisenstein rational reduction x = (a0 + a1 w) / (b0 + b1 w) of the FastPrime configuration"""
        am, bm = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        an, bn = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
        rc = self.lib.bppp_rational_reduce_eis(_ptr(int_to_limbs(x)), _ptr(am), C.c_void_p(an.ctypes.data), _ptr(bm), C.c_void_p(bn.ctypes.data))
        if rc != 0:
            raise BpppError(f"bppp_rational_reduce_eis failed ({rc})")
        comp = lambda m, s, k: (-1 if s[k] else 1) * (int(m[2 * k]) | (int(m[2 * k + 1]) << 64))
        return (comp(am, an, 0), comp(am, an, 1)), (comp(bm, bn, 0), comp(bm, bn, 1))

    def fold_points_eis(self, b, a, points: np.ndarray) -> np.ndarray:
        """out[j] = b * pts[2j] + a * pts[2j+1] for Eisenstein reduced scalars b = (b0, b1), a = (a0, a1)"""
        n = points.shape[0]
        mags = lambda e: np.array([abs(e[0]) & (2**64 - 1), abs(e[0]) >> 64, abs(e[1]) & (2**64 - 1), abs(e[1]) >> 64], dtype=np.uint64)
        negs = lambda e: np.array([int(e[0] < 0), int(e[1] < 0)], dtype=np.int32)
        d_p = self.to_device(np.ascontiguousarray(points))
        d_o = self.alloc(((n + 1) // 2) * 64)
        bn, an = negs(b), negs(a)
        try:
            self._check(self.lib.bppp_fold_points_eis_device(self.h, _ptr(mags(b)), C.c_void_p(bn.ctypes.data), _ptr(mags(a)), C.c_void_p(an.ctypes.data), _ptr(d_p), n,
                                                             _ptr(d_o)), "bppp_fold_points_eis_device")
            return self.download(d_o, ((n + 1) // 2, 8))
        finally:
            self.free(d_p); self.free(d_o)

    def fold_points(self, b: int, a: int, points: np.ndarray) -> np.ndarray:
        n = points.shape[0]
        out = np.zeros(((n + 1) // 2, 8), dtype=np.uint64)
        self._check(self.lib.bppp_fold_points(self.h, _ptr(int_to_limbs(abs(b), 3)), int(b < 0), _ptr(int_to_limbs(abs(a), 3)), int(a < 0),
                                              _ptr(np.ascontiguousarray(points)), n, _ptr(out)), "bppp_fold_points")
        return out

    def fold_points_device(self, b: int, a: int, d_points: int, n: int, d_out: int):
        self._check(self.lib.bppp_fold_points_device(self.h, _ptr(int_to_limbs(abs(b), 3)), int(b < 0), _ptr(int_to_limbs(abs(a), 3)), int(a < 0),
                                                     _ptr(d_points), n, _ptr(d_out)), "bppp_fold_points_device")

    # ---- round scalar kernels
    def norm_round_sums(self, d_x: int, n: int, q4: int) -> Tuple[int, int]:
        sx, sr = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        self._check(self.lib.bppp_norm_round_sums_device(self.h, _ptr(d_x), n, _ptr(int_to_limbs(q4)), _ptr(sx), _ptr(sr)), "bppp_norm_round_sums_device")
        return limbs_to_int(sx), limbs_to_int(sr)

    def lin_round_sums(self, d_c: int, d_x: int, n: int) -> Tuple[int, int]:
        sx, sr = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        self._check(self.lib.bppp_lin_round_sums_device(self.h, _ptr(d_c), _ptr(d_x), n, _ptr(sx), _ptr(sr)), "bppp_lin_round_sums_device")
        return limbs_to_int(sx), limbs_to_int(sr)

    def norm_round_openings(self, d_x: int, n: int, q: int, qinv: int, d_xw: int, d_rw: int):
        self._check(self.lib.bppp_norm_round_openings_device(self.h, _ptr(d_x), n, _ptr(int_to_limbs(q)), _ptr(int_to_limbs(qinv)), _ptr(d_xw), _ptr(d_rw)),
                    "bppp_norm_round_openings_device")

    def lin_round_openings(self, d_x: int, n: int, d_xw: int, d_rw: int):
        self._check(self.lib.bppp_lin_round_openings_device(self.h, _ptr(d_x), n, _ptr(d_xw), _ptr(d_rw)), "bppp_lin_round_openings_device")

    def fold_scalars(self, u: int, v: int, d_x: int, n: int, d_out: int):
        self._check(self.lib.bppp_fold_scalars_device(self.h, _ptr(int_to_limbs(u)), _ptr(int_to_limbs(v)), _ptr(d_x), n, _ptr(d_out)), "bppp_fold_scalars_device")

    def tensor(self, bs: Sequence[int], es: Sequence[int], qs: Sequence[int], d_out: int):
        k = len(es)
        assert len(qs) == k
        self._check(self.lib.bppp_tensor_device(self.h, _ptr(scalars_to_array(bs)), len(bs), _ptr(scalars_to_array(es)) if k else None,
                                                _ptr(scalars_to_array(qs)) if k else None, k, _ptr(d_out)), "bppp_tensor_device")

    def batch_inverse(self, d_x: int, n: int, modulus: int, d_out: int):
        self._check(self.lib.bppp_batch_inverse_device(self.h, _ptr(d_x), n, modulus, _ptr(d_out)), "bppp_batch_inverse_device")

    def lift_x(self, d_x: int, n: int, d_points: int):
        self._check(self.lib.bppp_lift_x_device(self.h, _ptr(d_x), n, _ptr(d_points)), "bppp_lift_x_device")

    # ---- a setup's basis from its seed (getPoints)
    def seed_candidate_x(self, seed: bytes, n: int) -> int:
        """bppp_seed_candidate_x (host only): x of candidate n of the seed's stream, before the curve test"""
        out = np.zeros(4, dtype=np.uint64)
        rc = self.lib.bppp_seed_candidate_x(bytes(seed), len(seed), n, _ptr(out))
        if rc != 0:
            raise BpppError(f"bppp_seed_candidate_x failed ({rc})")
        return limbs_to_int(out)

    def points_from_seed(self, seed: bytes, count: int, first_candidate: int = 0, device: bool = False):
        """`count` consecutive points of getPoints(seed), the search starting at candidate first_candidate: ((count, 8) uint64 array,
        next_candidate) — or, with device=True, (device pointer, next_candidate): the points stay in HBM (release with free())."""
        nxt = C.c_uint64(0)
        if device:
            d = self.alloc(max(count, 1) * 64)
            rc = self.lib.bppp_points_from_seed_device(self.h, bytes(seed), len(seed), first_candidate, count, _ptr(d), C.byref(nxt))
            if rc != 0:
                self.free(d)
            self._check(rc, "bppp_points_from_seed_device")
            return d, int(nxt.value)
        out = np.zeros((count, 8), dtype=np.uint64)
        self._check(self.lib.bppp_points_from_seed(self.h, bytes(seed), len(seed), first_candidate, count, C.c_void_p(out.ctypes.data), C.byref(nxt)),
                    "bppp_points_from_seed")
        return out, int(nxt.value)

    # ---- device memory
    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self.lib.bppp_device_alloc(self.h, nbytes, C.byref(p)), "bppp_device_alloc")
        return int(p.value)

    def free(self, d_ptr: int):
        self._check(self.lib.bppp_device_free(self.h, _ptr(d_ptr)), "bppp_device_free")

    def host_alloc(self, nbytes: int) -> np.ndarray:
        """page-locked host memory as a uint8 array (bppp_host_alloc): copies from it are DMA transfers; release with host_free"""
        p = C.c_void_p()
        self._check(self.lib.bppp_host_alloc(self.h, nbytes, C.byref(p)), "bppp_host_alloc")
        buf = (C.c_uint8 * max(nbytes, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8, count=nbytes)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr: np.ndarray):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is None:
            raise ValueError("not an array from host_alloc")
        self._check(self.lib.bppp_host_free(self.h, _ptr(p)), "bppp_host_free")

    def upload(self, d_dst: int, src: np.ndarray):
        src = np.ascontiguousarray(src)
        self._check(self.lib.bppp_upload(self.h, _ptr(d_dst), C.c_void_p(src.ctypes.data), src.nbytes), "bppp_upload")

    def download(self, d_src: int, shape, dtype=np.uint64) -> np.ndarray:
        out = np.zeros(shape, dtype=dtype)
        self._check(self.lib.bppp_download(self.h, C.c_void_p(out.ctypes.data), _ptr(d_src), out.nbytes), "bppp_download")
        return out

    def to_device(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = self.alloc(max(arr.nbytes, 16))
        if arr.nbytes:
            self.upload(p, arr)
        return p

    # ---- range proofs from HBM to HBM
    def rp_prove_batch_device(self, rp, batch: int, d_amounts: int, d_types: int, d_blinds: int, d_public_amounts: int, d_rand_prefix: int, prefix_len: int,
                              d_coms_files: int, d_proof_files: int):
        """bppp_rp_prove_batch_device: `rp` a bppp_rp handle, every buffer a device pointer (0 = NULL); the files are complete in HBM on return"""
        self._check(self.lib.bppp_rp_prove_batch_device(rp, batch, _ptr(d_amounts), _ptr(d_types), _ptr(d_blinds), _ptr(d_public_amounts), _ptr(d_rand_prefix),
                                                        prefix_len, _ptr(d_coms_files), _ptr(d_proof_files)), "bppp_rp_prove_batch_device")

    def rp_prove_batch_status_device(self, rp, batch: int, d_amounts: int, d_types: int, d_blinds: int, d_public_amounts: int, d_rand_prefix: int, prefix_len: int,
                                     d_coms_files: int, d_proof_files: int) -> np.ndarray:
        """bppp_rp_prove_batch_status_device: rp_prove_batch_device that refuses proof by proof; returns the RP_WIT_* verdicts (uint32 [batch]).  A
        refused proof's two files are zero bytes in HBM"""
        status = np.zeros(max(batch, 1), dtype=np.uint32)
        self._check(self.lib.bppp_rp_prove_batch_status_device(rp, batch, _ptr(d_amounts), _ptr(d_types), _ptr(d_blinds), _ptr(d_public_amounts), _ptr(d_rand_prefix),
                                                               prefix_len, _ptr(d_coms_files), _ptr(d_proof_files), C.c_void_p(status.ctypes.data)),
                    "bppp_rp_prove_batch_status_device")
        return status[:batch]

    # ---- profiling
    def profile_enable(self, on: bool = True):
        self._check(self.lib.bppp_profile_enable(self.h, int(on)), "bppp_profile_enable")

    def profile_read(self, reset: bool = True):
        ms = (C.c_double * NUM_STAGES)()
        calls = C.c_uint64(0)
        self._check(self.lib.bppp_profile_read(self.h, ms, C.byref(calls), int(reset)), "bppp_profile_read")
        return {STAGE_NAMES[k]: ms[k] for k in range(NUM_STAGES)}, int(calls.value)


class Basis:
    """bppp_basis: points registered once with their fixed-base table; msm() runs over the first n_terms of them."""

    def __init__(self, gpu: Bppp, points, window_bits: int = 0, batch_hint: int = 1, device: bool = False, n: int = 0):
        self.gpu, self.h = gpu, None
        h = C.c_void_p()
        if device:
            rc = gpu.lib.bppp_basis_create_device(gpu.h, _ptr(points), n, window_bits, batch_hint, C.byref(h))
        else:
            pts = np.ascontiguousarray(points)
            rc = gpu.lib.bppp_basis_create(gpu.h, _ptr(pts), pts.shape[0], window_bits, batch_hint, C.byref(h))
        gpu._check(rc, "bppp_basis_create")
        self.h = h
        gpu._adopt(self)
        n_, c_, tb = C.c_size_t(0), C.c_int(0), C.c_size_t(0)
        gpu._check(gpu.lib.bppp_basis_info(h, C.byref(n_), C.byref(c_), C.byref(tb)), "bppp_basis_info")
        self.n, self.window_bits, self.table_bytes = int(n_.value), int(c_.value), int(tb.value)

    def close(self):
        if self.h:
            self.gpu.lib.bppp_basis_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def enable_comb(self, window_bits: int = 0, budget_bytes: int = 32 << 30):
        """bppp_basis_enable_comb: keep every multiple of every window; returns (window_bits, table_bytes)"""
        c_, tb = C.c_int(0), C.c_size_t(0)
        self.gpu._check(self.gpu.lib.bppp_basis_enable_comb(self.h, window_bits, budget_bytes, C.byref(c_), C.byref(tb)), "bppp_basis_enable_comb")
        return int(c_.value), int(tb.value)

    def msm(self, d_scalars: int, n_terms: int, batch: int = 1):
        out = np.zeros((batch, 8), dtype=np.uint64)
        self.gpu._check(self.gpu.lib.bppp_msm_basis(self.h, _ptr(d_scalars), n_terms, batch, _ptr(out)), "bppp_msm_basis")
        return [array_to_point(out[b]) for b in range(batch)]
