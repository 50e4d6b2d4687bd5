"""ctypes binding of include/dagpu.h (libdagpu.so, built for gfx950).

The product path: every compute call goes through the HIP library.  If the
library is missing this module raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# DAGPU_LIB selects another build of the same library (A/B runs of kernel variants)
LIB_PATH = os.environ.get("DAGPU_LIB") or os.path.join(_PKG_ROOT, "libdagpu.so")

SHARE_SIZE = 512
NAMESPACE_SIZE = 29
ROOT_SIZE = 90
HASH_SIZE = 32

OK = 0
ERR_NOT_POW2 = -1
ERR_NOT_SQUARE = -2
ERR_SHARE_SIZE = -3
ERR_PUSH_ORDER = -4
ERR_TOO_FEW_SHARDS = -5
ERR_UNREPAIRABLE = -6
ERR_BYZANTINE = -7
ERR_BAD_ROOTS = -8
ERR_ARG = -9
ERR_DEVICE = -10
ERR_UNSUPPORTED = -11
ERR_PROOF = -12
ERR_SQUARE = -13

# Every symbol include/dagpu.h declares (checked by tests/test_abi_cpu.py).
EXPORTS = (
    "dagpu_version",
    "dagpu_max_square_width",
    "dagpu_max_codec_width",
    "dagpu_init",
    "dagpu_destroy",
    "dagpu_last_error",
    "dagpu_nmt_verify_inclusion",
    "dagpu_merkle_verify",
    "dagpu_nmt_verify_batch",
    "dagpu_nmt_verify_workspace_size",
    "dagpu_nmt_verify_batch_device",
    "dagpu_merkle_verify_batch",
    "dagpu_host_alloc",
    "dagpu_host_free",
    "dagpu_host_register",
    "dagpu_host_unregister",
    "dagpu_extend_shares",
    "dagpu_extend_batch",
    "dagpu_workspace_size",
    "dagpu_extend_batch_device",
    "dagpu_extend_rs_device",
    "dagpu_roots_device",
    "dagpu_roots",
    "dagpu_encode",
    "dagpu_decode",
    "dagpu_repair_workspace_size",
    "dagpu_repair_batch_device",
    "dagpu_repair_batch_device_ex",
    "dagpu_repair_start",
    "dagpu_repair_join",
    "dagpu_repair",
    "dagpu_repair_ex",
    "dagpu_square_construct",
    "dagpu_square_build",
    "dagpu_square_plan",
    "dagpu_square_plan_check",
    "dagpu_square_plan_write_host",
    "dagpu_square_write_workspace_size",
    "dagpu_square_write_device",
    "dagpu_square_plan_device_workspace_size",
    "dagpu_square_plan_device_arena_size",
    "dagpu_square_plan_device",
    "dagpu_square_construct_device",
    "dagpu_square_plan_emulate_host",
    "dagpu_blob_commitments_workspace_size",
    "dagpu_blob_commitments_device",
    "dagpu_square_plan_blobs",
    "dagpu_blob_tx_check",
    "dagpu_blob_tx_validate_workspace_size",
    "dagpu_blob_tx_validate_device",
    "dagpu_blob_tx_validate_host",
    "dagpu_commit_plan_table_words",
    "dagpu_commit_plan_workspace_size",
    "dagpu_commit_plan_device",
    "dagpu_commit_plan_host",
    "dagpu_proposal_check_workspace_size",
    "dagpu_proposal_check_device",
    "dagpu_proposal_verdict_workspace_size",
    "dagpu_proposal_verdict_device",
    "dagpu_proposal_verdict_host",
    "dagpu_secp256k1_verify_device",
    "dagpu_secp256k1_verify_host",
    "dagpu_secp256k1_g_table",
    "dagpu_tx_sig_verify_workspace_size",
    "dagpu_tx_signers_device",
    "dagpu_tx_signers_host",
    "dagpu_tx_sig_verify_device",
    "dagpu_tx_sig_verify_host",
    "dagpu_square_scan_workspace_size",
    "dagpu_square_scan_device",
    "dagpu_square_scan_host",
    "dagpu_square_read_workspace_size",
    "dagpu_square_read_device",
    "dagpu_compact_units",
    "dagpu_square_units_workspace_size",
    "dagpu_square_units_device",
    "dagpu_square_units_host",
    "dagpu_square_units_emulate_host",
    "dagpu_square_read_units_workspace_size",
    "dagpu_square_read_units_device",
    "dagpu_profile_enable",
    "dagpu_profile_read",
    "dagpu_profile_stages",
    "dagpu_repair_stats",
    "dagpu_dah_hash",
    "dagpu_nmt_roots",
    "dagpu_wrapper_roots",
    "dagpu_merkle_roots",
    "dagpu_merkle_levels",
    "dagpu_subtree_width",
    "dagpu_blob_commitments",
    "dagpu_split_workspace_size",
    "dagpu_split_rows_device",
    "dagpu_split_cols_device",
    "dagpu_split_finish_device",
    "dagpu_row_nodes_size",
    "dagpu_row_nodes_workspace_size",
    "dagpu_row_nodes_device",
    "dagpu_row_nodes_gather_device",
    "dagpu_col_nodes_size",
    "dagpu_col_nodes_workspace_size",
    "dagpu_col_nodes_device",
    "dagpu_nmt_prove_workspace_size",
    "dagpu_nmt_prove_batch_device",
    "dagpu_proof_store_size",
    "dagpu_proof_store_workspace_size",
    "dagpu_proof_store_device",
    "dagpu_nmt_prove_squares_workspace_size",
    "dagpu_nmt_prove_squares_device",
    "dagpu_share_proof_requests",
    "dagpu_nmt_verify_namespace",
    "dagpu_nmt_verify_namespace_batch",
    "dagpu_nmt_verify_namespace_workspace_size",
    "dagpu_nmt_verify_namespace_batch_device",
    "dagpu_nmt_namespace_workspace_size",
    "dagpu_nmt_namespace_ranges_device",
    "dagpu_nmt_prove_namespace_batch_device",
    "dagpu_nmt_namespace_squares_workspace_size",
    "dagpu_nmt_namespace_squares_count_device",
    "dagpu_nmt_prove_namespace_squares_device",
)

# d_status bits of dagpu_blob_commitments_device
COMMIT_MISMATCH = 1
COMMIT_PUSH_ORDER = 2

# dagpu_square_plan_device: status word = kind | index << 8
PLAN_OK, PLAN_NO_SPACE_TX, PLAN_NO_SPACE_BLOB_TX, PLAN_TX_AFTER_BLOB_TX = 0, 1, 2, 3
PLAN_LAYOUT, PLAN_TOO_MANY_BLOBS, PLAN_WIDTH, PLAN_ARENA = 4, 5, 6, 7
PLAN_RECORD_BYTES = 32
# dagpu_blob_tx_check / dagpu_blob_tx_validate_*: status word = kind | index << 8
# (DAGPU_BLOBTX_*; the names are blobtx.KIND_NAMES)
BLOBTX_KINDS = 25
BLOBTX_NONE = 0xFFFFFFFF
# dagpu_proposal_verdict_*: code of a block's record {code, tx, word, aux} (DAGPU_VERDICT_*)
VERDICT_NAMES = ("ACCEPT", "NON_BLOB_TX_HAS_PFB", "INVALID_BLOB_TX", "CALCULATE_COMMITMENT",
                 "INVALID_SHARE_COMMITMENT", "CONSTRUCT_FAILED", "SQUARE_SIZE_DIFFERS", "NOT_JUDGED", "EXTEND_FAILED",
                 "DATA_ROOT_DIFFERS")
COMMIT_COUNT_WORDS = 8
# dagpu_secp256k1_verify_* / dagpu_tx_sig_verify_*: status word = kind | index << 8 (DAGPU_SIG_*);
# kinds 1 .. 5 are not judged, kinds from 16 on reject
SIG_KIND_NAMES = {
    0: "SIG_OK", 1: "SIG_TX_UNDECODABLE", 2: "SIG_UNSUPPORTED_SIGNERS", 3: "SIG_UNSUPPORTED_MODE",
    4: "SIG_UNSUPPORTED_PUBKEY_TYPE", 5: "SIG_NO_PUBKEY", 16: "SIG_BAD_PUBKEY", 17: "SIG_BAD_LENGTH",
    18: "SIG_OUT_OF_RANGE", 19: "SIG_HIGH_S", 20: "SIG_MISMATCH"}
SIG_KINDS = {name: kind for kind, name in SIG_KIND_NAMES.items()}
SIG_REJECTING = 16
SIG_RECORD_BYTES = 136
SIGNER_RECORD_BYTES = 48
SIG_NONE = 0xFFFFFFFF
# dagpu_square_scan_device / dagpu_square_read_device (include/dagpu.h)
SCAN_OK, SCAN_NAMESPACE, SCAN_INCONSISTENT, SCAN_LENGTH, SCAN_OVERFLOW = 0, 1, 2, 3, 4
SCAN_SUMMARY_WORDS = 8
SEQ_SPARSE, SEQ_TX, SEQ_PFB, SEQ_PADDING, SEQ_VERSION_SHIFT = 1, 2, 4, 8, 8
SEQ_RECORD_BYTES = 64
READ_BLOBS, READ_COMPACT = 1, 2
# dagpu_square_units_device / dagpu_square_read_units_device
UNITS_OK, UNITS_SCAN, UNITS_HOST, UNITS_OVERFLOW = 0, 1, 2, 3
UNITS_SUMMARY_WORDS = 8
UNIT_RECORD_BYTES = 32
READ_UNITS_OVERFLOW, READ_UNITS_INVALID = 1, 2

PROVE_REQ_WORDS = 4
PROVE_SQ_REQ_WORDS = 5
MERKLE_DESC_WORDS = 6
NMT_DESC_WORDS = 8
NMT_NS_DESC_WORDS = 9
NS_OUTSIDE, NS_PRESENT, NS_ABSENT = 0, 1, 2
NS_HIT_WORDS = 6

PREFIX_NONE = 0
PREFIX_SELF = 1
PREFIX_PARITY = 2
PREFIX_FLAGS = 3

PROFILE_KERNELS = ("rs_row", "rs_col", "nmt_leaves", "nmt_trees", "dah", "decode", "repair_fill")
# dagpu_profile_stages (include/dagpu.h DAGPU_STAGE_*)
STAGES = ("start", "uploaded", "rs_rows", "rs_cols", "leaves", "trees", "dah", "results", "eds_top", "eds_bottom")

_lib = None

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
i32p = ctypes.POINTER(ctypes.c_int32)
vp = ctypes.c_void_p
sz = ctypes.c_size_t


class _Unbound:
    """Stand-in for an entry point an older build (DAGPU_LIB A/B runs) lacks."""

    def __init__(self, name):
        self.name = name

    def __call__(self, *a):
        raise AttributeError(f"{LIB_PATH}: no symbol {self.name}")


class _Tolerant:
    """An alternate build under A/B (DAGPU_LIB): symbols it lacks stay unbound."""

    def __init__(self, L):
        object.__setattr__(self, "_L", L)

    def __getattr__(self, name):
        try:
            return getattr(self._L, name)
        except AttributeError:
            u = _Unbound(name)
            object.__setattr__(self, name, u)
            return u


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"HIP extension not built: {LIB_PATH} missing (run __graft_entry__.build())")
        # Load PyTorch's bundled HIP runtime first when torch is installed:
        # libdagpu.so and torch then share ONE libamdhip64.so.7 (same soname).
        # Loading /opt/rocm's copy first would make torch bind to it and fail
        # its own device init ("No HIP GPUs are available").
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        if os.environ.get("DAGPU_LIB"):
            L = _Tolerant(L)
        L.dagpu_version.restype = ctypes.c_int
        L.dagpu_max_square_width.restype = ctypes.c_uint32
        L.dagpu_max_codec_width.restype = ctypes.c_uint32
        L.dagpu_init.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.dagpu_destroy.argtypes = [vp]
        L.dagpu_destroy.restype = None
        L.dagpu_last_error.argtypes = [vp]
        L.dagpu_last_error.restype = ctypes.c_char_p
        i64 = ctypes.c_int64
        L.dagpu_nmt_verify_inclusion.argtypes = [vp, vp, sz, sz, i64, i64, vp, sz, vp]
        L.dagpu_merkle_verify.argtypes = [vp, vp, sz, i64, i64, vp, sz]
        L.dagpu_nmt_verify_batch.argtypes = [vp, sz, vp, vp, sz, vp, sz, sz, vp, sz, vp, sz, vp]
        L.dagpu_nmt_verify_workspace_size.argtypes = [sz, sz]
        L.dagpu_nmt_verify_workspace_size.restype = sz
        L.dagpu_nmt_verify_batch_device.argtypes = [vp, sz, vp, vp, sz, vp, sz, sz, vp, sz, vp, sz, vp, vp, vp]
        L.dagpu_merkle_verify_batch.argtypes = [vp, sz, vp, vp, sz, sz, vp, vp, sz, vp, sz, vp]
        L.dagpu_host_alloc.argtypes = [sz]
        L.dagpu_host_alloc.restype = vp
        L.dagpu_host_free.argtypes = [vp]
        L.dagpu_host_free.restype = None
        L.dagpu_host_register.argtypes = [vp, sz]
        L.dagpu_host_unregister.argtypes = [vp]
        L.dagpu_extend_shares.argtypes = [vp, vp, sz, sz, vp, vp, vp, vp]
        L.dagpu_extend_batch.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp]
        L.dagpu_workspace_size.argtypes = [ctypes.c_uint32, sz]
        L.dagpu_workspace_size.restype = sz
        L.dagpu_extend_batch_device.argtypes = [vp, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, vp,
                                                vp, vp]
        L.dagpu_extend_rs_device.argtypes = [vp, ctypes.c_uint32, sz, vp, vp, vp]
        L.dagpu_roots_device.argtypes = [vp, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, vp, vp]
        L.dagpu_roots.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp]
        L.dagpu_encode.argtypes = [vp, ctypes.c_uint32, sz, sz, vp, vp]
        L.dagpu_decode.argtypes = [vp, ctypes.c_uint32, sz, sz, vp, vp]
        L.dagpu_repair_batch_device.argtypes = [vp, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, vp,
                                                vp]
        L.dagpu_repair_workspace_size.argtypes = [ctypes.c_uint32, sz]
        L.dagpu_repair_workspace_size.restype = sz
        L.dagpu_repair.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp]
        L.dagpu_profile_stages.argtypes = [vp, vp]
        L.dagpu_repair_stats.argtypes = [vp, vp]
        L.dagpu_repair_ex.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp]
        L.dagpu_square_construct.argtypes = [vp, vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, vp, sz, vp]
        L.dagpu_square_build.argtypes = [vp, vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, vp, sz, vp, vp]
        L.dagpu_square_plan.argtypes = [vp, vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, vp, vp, sz, vp, vp]
        L.dagpu_square_plan_check.argtypes = [vp, sz, sz]
        L.dagpu_square_plan_write_host.argtypes = [vp, sz, vp, sz, vp, sz]
        L.dagpu_square_write_workspace_size.argtypes = [sz, sz]
        L.dagpu_square_write_workspace_size.restype = sz
        L.dagpu_square_write_device.argtypes = [vp, ctypes.c_uint32, sz, vp, vp, vp, vp, sz, vp, sz, sz, vp, vp]
        for f in (L.dagpu_square_plan_device_workspace_size, L.dagpu_square_plan_device_arena_size):
            f.argtypes = [sz, sz, ctypes.c_uint32]
            f.restype = sz
        L.dagpu_square_plan_device.argtypes = [vp, sz, vp, vp, sz, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, sz,
                                               vp, vp, vp, vp]
        L.dagpu_square_construct_device.argtypes = [vp, ctypes.c_uint32, sz, vp, vp, sz, vp, vp, ctypes.c_uint32,
                                                    ctypes.c_uint32, vp, sz, vp, vp, sz, sz, vp, vp, vp]
        L.dagpu_square_plan_emulate_host.argtypes = [sz, vp, vp, sz, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, sz,
                                                     vp, vp]
        L.dagpu_blob_commitments_workspace_size.argtypes = [ctypes.c_uint32, sz, sz]
        L.dagpu_blob_commitments_workspace_size.restype = sz
        L.dagpu_blob_commitments_device.argtypes = [vp, ctypes.c_uint32, sz, sz, vp, vp, sz, sz, ctypes.c_uint32, vp, vp,
                                                    vp, vp, vp, vp]
        L.dagpu_square_plan_blobs.argtypes = [vp, sz, vp, sz, ctypes.POINTER(sz)]
        L.dagpu_blob_tx_check.argtypes = [vp, sz]
        L.dagpu_blob_tx_check.restype = ctypes.c_uint32
        L.dagpu_blob_tx_validate_workspace_size.argtypes = [sz, sz, sz]
        L.dagpu_blob_tx_validate_workspace_size.restype = sz
        L.dagpu_blob_tx_validate_device.argtypes = [vp, sz, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
        L.dagpu_blob_tx_validate_host.argtypes = [sz, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp]
        u32 = ctypes.c_uint32
        L.dagpu_commit_plan_table_words.argtypes = [u32, sz]
        L.dagpu_commit_plan_table_words.restype = sz
        L.dagpu_commit_plan_workspace_size.argtypes = [u32, sz]
        L.dagpu_commit_plan_workspace_size.restype = sz
        L.dagpu_commit_plan_device.argtypes = [vp, u32, sz, vp, sz, vp, u32, vp, vp, vp, vp, vp]
        L.dagpu_commit_plan_host.argtypes = [u32, sz, vp, sz, vp, u32, vp, vp, vp]
        L.dagpu_proposal_check_workspace_size.argtypes = [u32, sz, sz]
        L.dagpu_proposal_check_workspace_size.restype = sz
        L.dagpu_proposal_check_device.argtypes = [vp, u32, sz, vp, vp, sz, vp, vp, vp, sz, vp, vp, sz, sz, u32] + \
            [vp] * 11
        L.dagpu_proposal_verdict_workspace_size.argtypes = [u32, sz, sz]
        L.dagpu_proposal_verdict_workspace_size.restype = sz
        L.dagpu_proposal_verdict_device.argtypes = [vp, u32, sz] + [vp] * 12
        L.dagpu_proposal_verdict_host.argtypes = [u32, sz] + [vp] * 10
        L.dagpu_secp256k1_verify_device.argtypes = [vp, sz, vp, vp, vp, vp, vp]
        L.dagpu_secp256k1_verify_host.argtypes = [sz, vp, vp, vp, vp]
        L.dagpu_secp256k1_g_table.argtypes = [vp, ctypes.c_int]
        L.dagpu_tx_sig_verify_workspace_size.argtypes = [sz, sz]
        L.dagpu_tx_sig_verify_workspace_size.restype = sz
        L.dagpu_tx_signers_device.argtypes = [vp, sz, vp, vp, sz, vp, vp, vp, vp, vp]
        L.dagpu_tx_signers_host.argtypes = [sz, vp, vp, sz, vp, vp, vp]
        L.dagpu_tx_sig_verify_device.argtypes = [vp, sz, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
        L.dagpu_tx_sig_verify_host.argtypes = [sz, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp]
        L.dagpu_square_scan_workspace_size.argtypes = [u32, sz]
        L.dagpu_square_scan_workspace_size.restype = sz
        L.dagpu_square_scan_device.argtypes = [vp, u32, sz, vp, sz, sz, u32, vp, vp, vp, vp, vp]
        L.dagpu_square_scan_host.argtypes = [u32, sz, vp, sz, sz, u32, vp, vp]
        L.dagpu_square_read_workspace_size.argtypes = [u32, sz, u32, sz]
        L.dagpu_square_read_workspace_size.restype = sz
        L.dagpu_square_read_device.argtypes = [vp, u32, sz, vp, sz, sz, u32, vp, vp, vp, sz, u32, vp, vp, vp, vp, sz,
                                               vp, vp]
        L.dagpu_compact_units.argtypes = [vp, sz, u32, vp, vp, sz, ctypes.POINTER(sz)]
        L.dagpu_square_units_workspace_size.argtypes = [u32, sz]
        L.dagpu_square_units_workspace_size.restype = sz
        L.dagpu_square_units_device.argtypes = [vp, u32, sz, vp, sz, sz, u32, vp, vp, u32, vp, vp, vp, vp, vp]
        L.dagpu_square_units_host.argtypes = [u32, sz, vp, sz, sz, u32, vp, vp, u32, vp, vp]
        L.dagpu_square_units_emulate_host.argtypes = [u32, sz, vp, sz, sz, u32, vp, vp, u32, vp, vp]
        L.dagpu_square_read_units_workspace_size.argtypes = [sz]
        L.dagpu_square_read_units_workspace_size.restype = sz
        L.dagpu_square_read_units_device.argtypes = [vp, u32, sz, vp, sz, sz, u32, vp, u32, vp, vp, vp, sz, vp, vp, vp,
                                                     sz, vp, vp]
        L.dagpu_repair_batch_device_ex.argtypes = [vp, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, vp,
                                                   vp, vp]
        L.dagpu_repair_start.argtypes = [vp, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, vp, vp,
                                         ctypes.POINTER(ctypes.c_uint64)]
        L.dagpu_repair_join.argtypes = [vp, ctypes.c_uint64, vp]
        L.dagpu_dah_hash.argtypes = [vp, vp, sz, vp]
        L.dagpu_nmt_roots.argtypes = [vp, sz, vp, vp, sz, ctypes.c_int, vp, ctypes.c_int, vp, vp]
        L.dagpu_wrapper_roots.argtypes = [vp, ctypes.c_uint64, sz, vp, vp, vp, sz, vp, vp]
        L.dagpu_merkle_roots.argtypes = [vp, sz, vp, vp, sz, vp]
        L.dagpu_merkle_levels.argtypes = [vp, sz, vp, sz, vp, ctypes.POINTER(sz)]
        L.dagpu_subtree_width.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
        L.dagpu_blob_commitments.argtypes = [vp, sz, vp, vp, vp, ctypes.c_uint32, vp]
        L.dagpu_split_workspace_size.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        L.dagpu_split_workspace_size.restype = sz
        L.dagpu_split_rows_device.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp,
                                              vp, vp, vp]
        L.dagpu_split_cols_device.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp,
                                              vp, vp, vp, vp]
        L.dagpu_split_finish_device.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
        L.dagpu_row_nodes_size.argtypes = [ctypes.c_uint32]
        L.dagpu_row_nodes_size.restype = sz
        L.dagpu_row_nodes_workspace_size.argtypes = [ctypes.c_uint32]
        L.dagpu_row_nodes_workspace_size.restype = sz
        L.dagpu_row_nodes_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp]
        L.dagpu_row_nodes_gather_device.argtypes = [vp, ctypes.c_uint32, vp, sz, vp, vp, vp]
        L.dagpu_col_nodes_size.argtypes = [ctypes.c_uint32]
        L.dagpu_col_nodes_size.restype = sz
        L.dagpu_col_nodes_workspace_size.argtypes = [ctypes.c_uint32]
        L.dagpu_col_nodes_workspace_size.restype = sz
        L.dagpu_col_nodes_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp]
        L.dagpu_nmt_prove_workspace_size.argtypes = [sz]
        L.dagpu_nmt_prove_workspace_size.restype = sz
        L.dagpu_nmt_prove_batch_device.argtypes = [vp, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, sz, vp, vp, sz, vp,
                                                   ctypes.POINTER(sz), vp, vp]
        L.dagpu_proof_store_size.argtypes = [ctypes.c_uint32, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
        L.dagpu_proof_store_size.restype = sz
        L.dagpu_proof_store_workspace_size.argtypes = [ctypes.c_uint32, sz]
        L.dagpu_proof_store_workspace_size.restype = sz
        L.dagpu_proof_store_device.argtypes = [vp, ctypes.c_uint32, sz, vp, sz, vp, vp, vp]
        L.dagpu_nmt_prove_squares_workspace_size.argtypes = [sz]
        L.dagpu_nmt_prove_squares_workspace_size.restype = sz
        L.dagpu_nmt_prove_squares_device.argtypes = [vp, ctypes.c_uint32, sz, sz, vp, vp, sz, vp, vp, sz, vp, vp, sz,
                                                     vp, vp, vp, vp, vp, ctypes.POINTER(sz), vp, vp]
        L.dagpu_share_proof_requests.argtypes = [ctypes.c_uint32, sz, sz, vp, vp, sz, vp, ctypes.POINTER(sz)]
        L.dagpu_nmt_verify_namespace.argtypes = [vp, vp, sz, sz, i64, i64, vp, sz, vp, vp]
        L.dagpu_nmt_verify_namespace_batch.argtypes = [vp, sz, vp, vp, sz, vp, sz, sz, vp, sz, vp, sz, vp, sz, vp]
        L.dagpu_nmt_verify_namespace_workspace_size.argtypes = [sz, sz]
        L.dagpu_nmt_verify_namespace_workspace_size.restype = sz
        L.dagpu_nmt_verify_namespace_batch_device.argtypes = [vp, sz, vp, vp, sz, vp, sz, sz, vp, sz, vp, sz, vp, sz,
                                                              vp, vp, vp]
        L.dagpu_nmt_namespace_workspace_size.argtypes = [ctypes.c_uint32, sz]
        L.dagpu_nmt_namespace_workspace_size.restype = sz
        L.dagpu_nmt_namespace_ranges_device.argtypes = [vp, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, vp]
        L.dagpu_nmt_prove_namespace_batch_device.argtypes = [vp, ctypes.c_uint32, sz, vp, vp, vp, vp, sz, vp, vp, sz,
                                                             vp, sz, vp, vp, sz, vp, vp, vp]
        L.dagpu_nmt_namespace_squares_workspace_size.argtypes = [ctypes.c_uint32, sz, sz, sz]
        L.dagpu_nmt_namespace_squares_workspace_size.restype = sz
        L.dagpu_nmt_namespace_squares_count_device.argtypes = [vp, ctypes.c_uint32, sz, sz, vp, vp, vp, vp, vp, vp]
        L.dagpu_nmt_prove_namespace_squares_device.argtypes = [vp, ctypes.c_uint32, sz, sz, vp, vp, sz, vp, vp, sz,
                                                               vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp,
                                                               vp, vp]
        L.dagpu_profile_enable.argtypes = [vp, ctypes.c_int]
        L.dagpu_profile_read.argtypes = [vp, vp, vp, ctypes.c_int]
        _lib = L
    return _lib


def addr(buf) -> int:
    """Address of a numpy array / bytearray / torch tensor (device or host)."""
    if buf is None:
        return 0
    if hasattr(buf, "data_ptr"):
        return buf.data_ptr()
    if hasattr(buf, "ctypes"):
        return buf.ctypes.data
    if isinstance(buf, bytearray):
        return ctypes.addressof((ctypes.c_char * len(buf)).from_buffer(buf))
    raise TypeError(f"unsupported buffer type {type(buf)}")
