"""rust-eth-kzg_amd -- Python binding of the MI355X-native KZG engine (libc_eth_kzg.so).

Host-side mirror of the reference's `DASContext` API (reference: crates/eip7594/src/lib.rs:41-87,
prover.rs:100-171, verifier.rs:72-112) over the drop-in C ABI declared in include/c_eth_kzg.h.
Same method names, argument meaning and error behaviour as the reference bindings: an operation
that the reference reports as `Err` raises `KzgError`; `verify_cell_kzg_proof_batch` returns False
for an invalid proof and raises for malformed input.

There is NO CPU fallback: importing works without a GPU, but creating a context requires the HIP
library built by `rust-eth-kzg_amd/csrc/Makefile` and a gfx950 device, and fails loudly otherwise.

(The directory name contains a hyphen, so load it with importlib:
    kzg = importlib.import_module("rust-eth-kzg_amd") )
"""
import ctypes as C

import numpy as np
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libc_eth_kzg.so")  # the product library: what a maintainer links
HOOKS_LIB_PATH = os.path.join(_HERE, "libc_eth_kzg_hooks.so")  # the same objects + the stage-level test hooks: what tests/ loads

BYTES_PER_BLOB = 131072
BYTES_PER_CELL = 2048
BYTES_PER_COMMITMENT = 48
BYTES_PER_PROOF = 48
CELLS_PER_EXT_BLOB = 128
FIELD_ELEMENTS_PER_BLOB = 4096
FIELD_ELEMENTS_PER_CELL = 64


class KzgError(Exception):
    """An operation the reference would report as `Err(..)` (CResult.status == Err)."""


class CResult(C.Structure):
    _fields_ = [("status", C.c_int), ("error_msg", C.c_void_p)]


# every symbol include/c_eth_kzg.h declares (tests assert the library exports all of them)
VERIFY_PARTIAL_BYTES = 96
# flags of eth_kzg_amd_das_context_new_with_setup
SETUP_NO_SUBGROUP_CHECK = 1
SETUP_CHECK_POWERS = 2
SETUP_G1_POINTS = 4096
SETUP_G2_POINTS = 65
# flags of eth_kzg_amd_verify_cell_kzg_proof_batch_ex / _device_ex / _many_ex / _many_device_ex
VERIFY_LEAF_TRANSCRIPT = 1
# flag of eth_kzg_amd_blobs_to_data_columns / _device
COLUMNS_VERIFY_PROOFS = 1

EXPORTED_SYMBOLS = [
    "eth_kzg_das_context_new", "eth_kzg_das_context_free", "eth_kzg_free_error_message",
    "eth_kzg_blob_to_kzg_commitment", "eth_kzg_compute_cells_and_kzg_proofs", "eth_kzg_compute_cells",
    "eth_kzg_verify_cell_kzg_proof_batch", "eth_kzg_recover_cells_and_proofs",
    "eth_kzg_constant_bytes_per_cell", "eth_kzg_constant_bytes_per_proof", "eth_kzg_constant_cells_per_ext_blob",
    "eth_kzg_compute_kzg_proof", "eth_kzg_compute_blob_kzg_proof", "eth_kzg_verify_kzg_proof",
    "eth_kzg_verify_blob_kzg_proof", "eth_kzg_verify_blob_kzg_proof_batch",
    "eth_kzg_amd_das_context_new_on_device",
    "eth_kzg_amd_das_context_try_new", "eth_kzg_amd_das_context_new_on_devices", "eth_kzg_amd_context_devices",
    "eth_kzg_amd_das_context_new_with_setup", "eth_kzg_amd_das_context_new_with_setup_file", "eth_kzg_amd_setup_digest",
    "eth_kzg_amd_abi_version", "eth_kzg_amd_window_count", "eth_kzg_amd_glv_table",
    "eth_kzg_amd_compute_cells_and_kzg_proofs_batch", "eth_kzg_amd_blob_to_kzg_commitment_batch",
    "eth_kzg_amd_recover_cells_and_proofs_batch", "eth_kzg_amd_recover_cells_and_proofs_device",
    "eth_kzg_amd_verify_cell_kzg_proof_batch_partial", "eth_kzg_amd_verify_cell_kzg_proof_batch_combine",
    "eth_kzg_amd_compute_cells_and_kzg_proofs_device", "eth_kzg_amd_blob_to_kzg_commitment_device",
    "eth_kzg_amd_verify_cell_kzg_proof_batch_device", "eth_kzg_amd_verify_cell_kzg_proof_batch_many",
    "eth_kzg_amd_verify_cell_kzg_proof_batch_ex", "eth_kzg_amd_verify_cell_kzg_proof_batch_device_ex",
    "eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex", "eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex",
    "eth_kzg_amd_compute_blob_kzg_proof_batch", "eth_kzg_amd_compute_kzg_proof_batch",
    "eth_kzg_amd_compute_blob_kzg_proof_device", "eth_kzg_amd_compute_kzg_proof_device",
    "eth_kzg_amd_verify_blob_kzg_proof_batch_device",
    "eth_kzg_amd_verify_kzg_proof_many", "eth_kzg_amd_verify_kzg_proof_many_device",
    "eth_kzg_amd_verify_blob_kzg_proof_many", "eth_kzg_amd_verify_blob_kzg_proof_many_device",
    "eth_kzg_amd_verify_data_columns", "eth_kzg_amd_verify_data_columns_device",
    "eth_kzg_amd_verify_partial_data_columns", "eth_kzg_amd_verify_partial_data_columns_device",
    "eth_kzg_amd_verify_blob_cell_proofs_many", "eth_kzg_amd_verify_blob_cell_proofs_many_device",
    "eth_kzg_amd_compute_data_columns", "eth_kzg_amd_compute_data_columns_device",
    "eth_kzg_amd_blobs_to_data_columns", "eth_kzg_amd_blobs_to_data_columns_device",
    "eth_kzg_amd_recover_data_columns", "eth_kzg_amd_recover_data_columns_device",
    "eth_kzg_amd_recover_data_columns_checked", "eth_kzg_amd_recover_data_columns_checked_device",
    "eth_kzg_amd_table_bytes", "eth_kzg_amd_window_bits", "eth_kzg_amd_tables_ready", "eth_kzg_amd_table_groups_ready", "eth_kzg_amd_table_build_info", "eth_kzg_amd_linmap_info",
    "eth_kzg_amd_set_profiling", "eth_kzg_amd_get_stage_times",
    "eth_kzg_amd_comm_probe", "eth_kzg_amd_comm_unique_id", "eth_kzg_amd_comm_init", "eth_kzg_amd_comm_info",
    "eth_kzg_amd_all_gather", "eth_kzg_amd_comm_destroy",
    "eth_kzg_amd_compute_cells_and_kzg_proofs_batch_multi", "eth_kzg_amd_device_count",
]
# include/c_eth_kzg_test_hooks.h: stage-level hooks for tests/, not part of the drop-in ABI
TEST_HOOK_SYMBOLS = [
    "eth_kzg_amd_test_fr_ntt4096", "eth_kzg_amd_test_g1_fft128", "eth_kzg_amd_test_fixed_msm", "eth_kzg_amd_test_fixed_msm_ex",
    "eth_kzg_amd_test_g1_decompress", "eth_kzg_amd_test_field_mul", "eth_kzg_amd_test_op_info", "eth_kzg_amd_test_op",
    "eth_kzg_amd_test_table_info", "eth_kzg_amd_test_table_audit", "eth_kzg_amd_test_table_read", "eth_kzg_amd_test_table_audit_buffer",
    "eth_kzg_amd_test_sha256_many", "eth_kzg_amd_test_verify_msm",
    "eth_kzg_amd_test_verify_cells_partial_device", "eth_kzg_amd_test_verify_blob_batch_inputs", "eth_kzg_amd_test_rs_decode",
    "eth_kzg_amd_test_prover_scalars", "eth_kzg_amd_test_verify_many_sums",
    "eth_kzg_amd_test_proofs_from_sums", "eth_kzg_amd_test_linmap_program",
    "eth_kzg_amd_test_cell_leaf_digests", "eth_kzg_amd_test_verify_cells_inputs_ex",
    "eth_kzg_amd_test_verify_many_sums_ex", "eth_kzg_amd_test_verify_many_sums_device",
    "eth_kzg_amd_test_verify_kzg_proof_many_sums",
    "eth_kzg_amd_test_blob_eval_at", "eth_kzg_amd_test_verify_blob_kzg_proof_many_sums",
    "eth_kzg_amd_test_pairing_check_many", "eth_kzg_amd_test_search_stats", "eth_kzg_amd_test_g1_decode",
    "eth_kzg_amd_test_verify_data_columns_sums", "eth_kzg_amd_test_verify_partial_data_columns_sums",
    "eth_kzg_amd_test_blob_extension", "eth_kzg_amd_test_verify_blob_cell_proofs_sums",
    "eth_kzg_amd_test_blob_to_columns",
]

_lib = None


def load_library():
    """dlopen libc_eth_kzg.so and declare the prototypes. Raises if the HIP extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("ETH_KZG_AMD_LIB", LIB_PATH)  # A/B builds of the same library (tools/); default: the in-tree build
    if not os.path.exists(path):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C rust-eth-kzg_amd/csrc). There is no CPU fallback.")
    lib = C.CDLL(path)
    P, U8P, U64 = C.c_void_p, C.c_char_p, C.c_uint64
    lib.eth_kzg_das_context_new.restype = P
    lib.eth_kzg_das_context_new.argtypes = [C.c_bool]
    lib.eth_kzg_amd_das_context_new_on_device.restype = P
    lib.eth_kzg_amd_das_context_new_on_device.argtypes = [C.c_bool, C.c_int]
    lib.eth_kzg_amd_das_context_try_new.restype = P
    lib.eth_kzg_amd_das_context_try_new.argtypes = [C.c_bool, C.c_int, C.c_double, C.POINTER(CResult)]
    lib.eth_kzg_das_context_free.argtypes = [P]
    lib.eth_kzg_free_error_message.argtypes = [P]
    for name, args in {
        "eth_kzg_blob_to_kzg_commitment": [P, U8P, P],
        "eth_kzg_compute_cells_and_kzg_proofs": [P, U8P, P, P],
        "eth_kzg_compute_cells": [P, U8P, P],
        "eth_kzg_verify_cell_kzg_proof_batch": [P, U64, P, U64, P, U64, P, U64, P, P],
        "eth_kzg_recover_cells_and_proofs": [P, U64, P, U64, P, P, P],
        "eth_kzg_compute_kzg_proof": [P, U8P, U8P, P, P],
        "eth_kzg_compute_blob_kzg_proof": [P, U8P, U8P, P],
        "eth_kzg_verify_kzg_proof": [P, U8P, U8P, U8P, U8P, P],
        "eth_kzg_verify_blob_kzg_proof": [P, U8P, U8P, U8P, P],
        "eth_kzg_verify_blob_kzg_proof_batch": [P, U64, P, U64, P, U64, P, P],
        "eth_kzg_amd_compute_cells_and_kzg_proofs_batch": [P, U64, P, P, P, P],
        "eth_kzg_amd_blob_to_kzg_commitment_batch": [P, U64, P, P, P],
        "eth_kzg_amd_recover_cells_and_proofs_batch": [P, U64, P, P, P, P, P, P, P],
        "eth_kzg_amd_verify_cell_kzg_proof_batch_partial": [P, U64, P, U64, P, U64, P, U64, P, U64, U64, P],
        "eth_kzg_amd_verify_cell_kzg_proof_batch_combine": [P, U64, U8P, P],
        "eth_kzg_amd_recover_cells_and_proofs_device": [P, U64, P, P, P, P, P, P],
        "eth_kzg_amd_compute_cells_and_kzg_proofs_device": [P, U64, P, P, P, P, P],
        "eth_kzg_amd_blob_to_kzg_commitment_device": [P, U64, P, P, P, P],
        "eth_kzg_amd_verify_cell_kzg_proof_batch_device": [P, U64, P, P, P, P, P, P],
        "eth_kzg_amd_verify_cell_kzg_proof_batch_many": [P, U64, P, P, P, P, P, P, P, P, P, P],
        "eth_kzg_amd_compute_blob_kzg_proof_batch": [P, U64, P, P, P, P],
        "eth_kzg_amd_compute_kzg_proof_batch": [P, U64, P, P, P, P, P],
        "eth_kzg_amd_compute_blob_kzg_proof_device": [P, U64, P, P, P, P, P],
        "eth_kzg_amd_compute_kzg_proof_device": [P, U64, P, P, P, P, P, P],
        "eth_kzg_amd_verify_blob_kzg_proof_batch_device": [P, U64, P, P, P, P, P],
        "eth_kzg_amd_comm_unique_id": [P],
        "eth_kzg_amd_comm_probe": [P, P, U64],
        "eth_kzg_amd_comm_info": [P, P, P],
        "eth_kzg_amd_comm_init": [P, U8P, C.c_int, C.c_int],
        "eth_kzg_amd_all_gather": [P, P, P, U64, P],
        "eth_kzg_amd_compute_cells_and_kzg_proofs_batch_multi": [P, U64, U64, P, P, P, P],
    }.items():
        fn = getattr(lib, name)
        fn.restype = CResult
        fn.argtypes = args
    for name in ("eth_kzg_constant_bytes_per_cell", "eth_kzg_constant_bytes_per_proof",
                 "eth_kzg_constant_cells_per_ext_blob"):
        getattr(lib, name).restype = U64
    lib.eth_kzg_amd_comm_destroy.argtypes = [P]
    lib.eth_kzg_amd_comm_destroy.restype = None
    lib.eth_kzg_amd_device_count.restype = C.c_int
    lib.eth_kzg_amd_table_bytes.restype = U64
    lib.eth_kzg_amd_table_bytes.argtypes = [P]
    lib.eth_kzg_amd_window_bits.argtypes = [P]
    lib.eth_kzg_amd_tables_ready.argtypes = [P, C.c_int]
    lib.eth_kzg_amd_tables_ready.restype = C.c_int
    lib.eth_kzg_amd_table_build_info.argtypes = [P, C.POINTER(C.c_double)]
    lib.eth_kzg_amd_table_build_info.restype = None
    lib.eth_kzg_amd_table_groups_ready.argtypes = [P]
    lib.eth_kzg_amd_table_groups_ready.restype = C.c_int
    lib.eth_kzg_amd_linmap_info.argtypes = [P, P]
    lib.eth_kzg_amd_linmap_info.restype = None
    lib.eth_kzg_amd_set_profiling.argtypes = [P, C.c_int]
    lib.eth_kzg_amd_set_profiling.restype = None
    lib.eth_kzg_amd_get_stage_times.argtypes = [P, P, P, C.c_int]
    lib.eth_kzg_amd_das_context_new_on_devices.restype = P
    lib.eth_kzg_amd_das_context_new_on_devices.argtypes = [C.c_bool, P, U64, C.c_double, C.POINTER(CResult)]
    lib.eth_kzg_amd_context_devices.restype = U64
    lib.eth_kzg_amd_context_devices.argtypes = [P, P, U64]
    lib.eth_kzg_amd_abi_version.restype = C.c_int
    if hasattr(lib, "eth_kzg_amd_das_context_new_with_setup"):  # (an A/B build from before these symbols, via ETH_KZG_AMD_LIB, still loads; calling them there raises)
        lib.eth_kzg_amd_das_context_new_with_setup.restype = P
        lib.eth_kzg_amd_das_context_new_with_setup.argtypes = [P, U64, P, U64, C.c_uint32, C.c_bool, P, U64, C.c_double, C.POINTER(CResult)]
        lib.eth_kzg_amd_das_context_new_with_setup_file.restype = P
        lib.eth_kzg_amd_das_context_new_with_setup_file.argtypes = [P, U64, C.c_uint32, C.c_bool, P, U64, C.c_double, C.POINTER(CResult)]
        lib.eth_kzg_amd_setup_digest.restype = None
        lib.eth_kzg_amd_setup_digest.argtypes = [P, P]
    for name, args in {
        "eth_kzg_amd_verify_cell_kzg_proof_batch_ex": [P, U64, P, U64, P, U64, P, U64, P, C.c_uint32, P],
        "eth_kzg_amd_verify_cell_kzg_proof_batch_device_ex": [P, U64, P, P, P, P, C.c_uint32, P, P],
        "eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex": [P, U64, P, P, P, P, P, P, P, P, C.c_uint32, P, P],
        "eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex": [P, U64, P, P, P, P, P, C.c_uint32, P, P, P],
        "eth_kzg_amd_verify_kzg_proof_many": [P, U64, P, P, P, P, P, P],
        "eth_kzg_amd_verify_kzg_proof_many_device": [P, U64, P, P, P, P, P, P, P],
        "eth_kzg_amd_verify_blob_kzg_proof_many": [P, U64, P, P, P, P, P],
        "eth_kzg_amd_verify_blob_kzg_proof_many_device": [P, U64, P, P, P, P, P, P],
        "eth_kzg_amd_verify_data_columns": [P, U64, P, U64, P, P, P, C.c_uint32, P, P],
        "eth_kzg_amd_verify_blob_cell_proofs_many": [P, U64, P, P, P, P, P],
        "eth_kzg_amd_verify_blob_cell_proofs_many_device": [P, U64, P, P, P, P, P, P],
        "eth_kzg_amd_verify_data_columns_device": [P, U64, P, U64, P, P, P, C.c_uint32, P, P, P],
        "eth_kzg_amd_verify_partial_data_columns": [P, U64, P, U64, P, P, P, P, C.c_uint32, P, P],
        "eth_kzg_amd_verify_partial_data_columns_device": [P, U64, P, U64, P, P, P, P, C.c_uint32, P, P, P],
        "eth_kzg_amd_compute_data_columns": [P, U64, P, P, P, P, P],
        "eth_kzg_amd_compute_data_columns_device": [P, U64, P, P, P, P, P, P],
        "eth_kzg_amd_blobs_to_data_columns": [P, U64, P, P, P, C.c_uint32, P, P, P, P],
        "eth_kzg_amd_blobs_to_data_columns_device": [P, U64, P, P, P, C.c_uint32, P, P, P, P, P],
        "eth_kzg_amd_recover_data_columns": [P, U64, U64, P, P, P, P, P],
        "eth_kzg_amd_recover_data_columns_device": [P, U64, U64, P, P, P, P, P, P],
        "eth_kzg_amd_recover_data_columns_checked": [P, U64, P, U64, P, P, P, P, P, P, P],
        "eth_kzg_amd_recover_data_columns_checked_device": [P, U64, P, U64, P, P, P, P, P, P, P, P],
    }.items():
        if hasattr(lib, name):  # (as above: a build from before these symbols still loads)
            getattr(lib, name).restype = CResult
            getattr(lib, name).argtypes = args
    lib.eth_kzg_amd_window_count.argtypes = [P]
    lib.eth_kzg_amd_glv_table.argtypes = [P]
    # the stage-level test hooks exist in libc_eth_kzg_hooks.so only (what tests/ loads through ETH_KZG_AMD_LIB); the product
    # library does not export them
    for name, args in {
        "eth_kzg_amd_test_fr_ntt4096": [P, U8P, P, C.c_int],
        "eth_kzg_amd_test_g1_fft128": [P, U8P, P, C.c_int, C.c_int],
        "eth_kzg_amd_test_fixed_msm": [P, U8P, C.c_int, P],
        "eth_kzg_amd_test_fixed_msm_ex": [P, C.c_int, C.c_int, C.c_int, P, C.c_int, P, P],
        "eth_kzg_amd_test_g1_decompress": [P, U8P, C.c_int, C.c_int, P, P],
        "eth_kzg_amd_test_g1_decode": [P, C.c_int, U8P, C.c_int, C.c_int, P, P],
        "eth_kzg_amd_test_field_mul": [P, U8P, U8P, P, C.c_int, C.c_int],
        "eth_kzg_amd_test_op_info": [C.c_int, P, P, P, C.POINTER(C.c_char_p)],
        "eth_kzg_amd_test_op": [P, C.c_int, C.c_int, P, P, C.c_int],
        "eth_kzg_amd_test_table_info": [P, C.c_int, C.c_int, P, P, C.c_int],
        "eth_kzg_amd_test_table_audit": [P, C.c_int, C.c_int, P, P, P, C.c_int, P],
        "eth_kzg_amd_test_table_read": [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P],
        "eth_kzg_amd_test_table_audit_buffer": [P, C.c_int, C.c_int, C.c_int, P, P, C.c_int, P, P, P, C.c_int],
        "eth_kzg_amd_test_sha256_many": [P, U64, P, U64, P, U64, U64, P, U64, U64, P],
        "eth_kzg_amd_test_verify_msm": [P, C.c_int, U8P, C.c_int, U8P, C.c_int, U8P, C.c_int, P, P],
        "eth_kzg_amd_test_verify_cells_partial_device": [P, U64, P, P, P, P, U64, U64, P],
        "eth_kzg_amd_test_verify_blob_batch_inputs": [P, U64, C.c_int, P, P, P, P, P],
        "eth_kzg_amd_test_rs_decode": [P, C.c_int, P, P, P, C.c_int, P, P, P, P, P, P],
        "eth_kzg_amd_test_prover_scalars": [P, C.c_int, P, P, U64, P, P, P, P, P],
        "eth_kzg_amd_test_verify_many_sums": [P, U64, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, U64, P],
        "eth_kzg_amd_test_proofs_from_sums": [P, C.c_int, C.c_int, P, P],
        "eth_kzg_amd_test_linmap_program": [P, C.c_int, P, U64, P, P, U64, P, P, P, U64, P],
        "eth_kzg_amd_test_cell_leaf_digests": [P, U64, P, P, P, P, P],
        "eth_kzg_amd_test_verify_cells_inputs_ex": [P, U64, C.c_int, P, P, P, P, C.c_uint32, P, P],
        "eth_kzg_amd_test_verify_many_sums_ex": [P, U64, P, P, P, P, P, P, P, P, C.c_uint32, P, P, P, P, P, P, P, P, U64, P, P, P],
        "eth_kzg_amd_test_verify_many_sums_device": [P, U64, P, P, P, P, P, C.c_uint32, P, P, P, P, P, P, P, P, U64, P, P, P],
        "eth_kzg_amd_test_verify_kzg_proof_many_sums": [P, U64, C.c_int, P, P, P, P, U64, P, P, P, U64, P, P, P, P, P, P, P, P, U64, P],
        "eth_kzg_amd_test_blob_eval_at": [P, U64, P, P, P, P],
        "eth_kzg_amd_test_pairing_check_many": [P, C.c_int, U64, P, C.c_int, P, P, P, P],
        "eth_kzg_amd_test_search_stats": [P, P],
        "eth_kzg_amd_test_verify_blob_kzg_proof_many_sums": [P, U64, C.c_int, P, P, P, U64, P, P, P, U64, P, P, P, P, P, P, P, P, U64, P, P, P],
        "eth_kzg_amd_test_verify_data_columns_sums": [P, U64, C.c_int, P, U64, P, P, P, C.c_uint32, P, P, P, P, P, P, P, P, U64, P, P, P, P],
        "eth_kzg_amd_test_verify_partial_data_columns_sums": [P, U64, C.c_int, P, U64, P, P, P, P, C.c_uint32, P, P, P, P, P, P, P, P, U64, P, P, P, P],
        "eth_kzg_amd_test_blob_extension": [P, U64, P, P, P],
        "eth_kzg_amd_test_blob_to_columns": [P, U64, P, U64, U64, C.c_int, P, P],
        "eth_kzg_amd_test_verify_blob_cell_proofs_sums": [P, U64, C.c_int, P, P, P, P, P, P, P, P, P, P, P, U64, P, P, P],
    }.items():
        if hasattr(lib, name):
            getattr(lib, name).argtypes = args
    _lib = lib
    return lib


def present_masks(n, present):
    """Two 64-bit words per blob for eth_kzg_amd_recover_cells_and_proofs_device: bit (c % 64) of word (c / 64) set when
    cell c of that blob carries data.  present[b] = iterable of cell indices (lists, tuples, rows of a 2-D array ...)."""
    masks = np.zeros(2 * max(1, n), dtype=np.uint64)
    # the same index list for many blobs (the usual case: [idx] * n) is folded into its mask once.  The cache holds the
    # row OBJECT and compares with `is`: an id() of a temporary (a row of a 2-D numpy array is a fresh view per access)
    # can be reused by the next row once the temporary is freed, which would silently give every blob the first mask.
    prev_row, prev_mask = None, 0
    for b in range(n):
        row = present[b]
        if row is prev_row and prev_row is not None:
            m = prev_mask
        else:
            m = 0
            for c in row:
                c = int(c)
                if not 0 <= c < CELLS_PER_EXT_BLOB:
                    raise KzgError("InvalidCellIndex")
                m |= 1 << c
            prev_row, prev_mask = row, m
        masks[2 * b] = m & 0xFFFFFFFFFFFFFFFF
        masks[2 * b + 1] = m >> 64
    return masks


def parse_trusted_setup_json(text):
    """The consensus-specs trusted-setup JSON -> (g1_monomial, g2_monomial) as lists of bytes (48 and 96 bytes each).
    Every entry is a 0x-prefixed hex string; `g1_lagrange` is not needed and ignored, as in the reference
    (crates/trusted_setup/src/lib.rs:111).  Raises KzgError on anything else; the point COUNTS are the constructor's business."""
    import json
    try:
        doc = json.loads(text)
    except ValueError as e:
        raise KzgError(f"InvalidSetup: not JSON ({e})")
    if not isinstance(doc, dict):
        raise KzgError("InvalidSetup: the trusted setup JSON is an object with g1_monomial and g2_monomial")
    out = []
    for key, size in (("g1_monomial", 48), ("g2_monomial", 96)):
        pts = doc.get(key)
        if not isinstance(pts, list):
            raise KzgError(f"InvalidSetup: {key} is missing")
        dec = []
        for i, h in enumerate(pts):
            if not isinstance(h, str) or not h.startswith("0x"):
                raise KzgError(f"InvalidSetup: {key}[{i}] is not a 0x-prefixed hex string")
            try:
                b = bytes.fromhex(h[2:])
            except ValueError:
                raise KzgError(f"InvalidSetup: {key}[{i}] is not hex")
            if len(b) != size:
                raise KzgError(f"InvalidSetup: {key}[{i}] has {len(b)} bytes, not {size}")
            dec.append(b)
        out.append(dec)
    return out[0], out[1]


def _ptr_array(bufs):
    """(array of char*, keep-alive list) over a list of bytes / ctypes buffers."""
    arr = (C.c_void_p * max(1, len(bufs)))()
    keep = []
    for i, b in enumerate(bufs):
        if isinstance(b, (bytes, bytearray)):
            b = C.create_string_buffer(bytes(b), len(b))
        keep.append(b)
        arr[i] = C.addressof(b)
    return arr, keep


def _flat_ptrs(items, size):
    """(uint64 pointer table, keep-alive) over ONE contiguous copy of equal-length byte strings: marshalling thousands
    of cells through per-item ctypes buffers costs more than the GPU work it feeds."""
    n = len(items)
    flat = np.frombuffer(b"".join(bytes(x) if not isinstance(x, bytes) else x for x in items), dtype=np.uint8) if n else np.zeros(1, np.uint8)
    ptrs = np.uint64(flat.ctypes.data) + np.arange(max(1, n), dtype=np.uint64) * np.uint64(size)
    return ptrs, flat


def _alias_ptrs(items):
    """(uint64 pointer table, keep-alive) over byte strings WITHOUT copying them together: equal objects share one buffer, so a list
    that names a few 128 KB blobs many times costs those few."""
    bufs, ptrs = {}, np.zeros(max(1, len(items)), dtype=np.uint64)
    for i, x in enumerate(items):
        key = id(x)
        if key not in bufs:
            a = np.frombuffer(x if isinstance(x, bytes) else bytes(x), dtype=np.uint8)
            bufs[key] = (a, x)  # (the object stays alive with its id)
        ptrs[i] = bufs[key][0].ctypes.data
    return ptrs, bufs


def _out_ptrs(n_outer, n_inner, size):
    """Caller-allocated outputs as one flat buffer: (flat uint8 array, inner pointer tables [n_outer][n_inner],
    outer pointer table [n_outer]) in the layout the C ABI takes (arrays of n_inner pointers per blob)."""
    flat = np.zeros(max(1, n_outer * n_inner * size), dtype=np.uint8)
    inner = np.uint64(flat.ctypes.data) + np.arange(max(1, n_outer * n_inner), dtype=np.uint64) * np.uint64(size)
    outer = np.uint64(inner.ctypes.data) + np.arange(max(1, n_outer), dtype=np.uint64) * np.uint64(n_inner * 8)
    return flat, inner, outer


def _split(flat, n_outer, n_inner, size):
    raw = flat.tobytes()
    return [[raw[(b * n_inner + k) * size:(b * n_inner + k + 1) * size] for k in range(n_inner)] for b in range(n_outer)]


def _vp(arr):
    return arr.ctypes.data_as(C.c_void_p)


class DASContext:
    """Mirror of `rust_eth_kzg::DASContext` (crates/eip7594/src/lib.rs:41-87)."""

    device_index = 0

    def __init__(self, use_precomp=True, device=None, wait_tables=True, table_budget_gb=None, devices=None):
        """devices: a device LIST -- one engine per listed GPU behind this one context (eth_kzg_amd_das_context_new_on_devices:
        single calls go to the least-loaded device, batched calls are cut into contiguous slices); ordinals may repeat.
        table_budget_gb: HBM for the two window tables together (None: $ETH_KZG_AMD_TABLE_GB or the library's default of 108 GB;
        a negative number: whatever the HBM holds) -- given, the context is made by eth_kzg_amd_das_context_try_new, which reports a
        failure as KzgError instead of aborting the process.
        wait_tables: the C entry point returns as soon as the start tables are up (progressive start); by default this
        wrapper then waits for the wide tables, so that timing and table introspection see the final state.  Pass False to
        use the context at once (results are identical on every table)."""
        self.device_index = int(device) if device is not None else int(os.environ.get("ETH_KZG_AMD_DEVICE", "0"))
        self._lib = load_library()
        if devices is not None:
            devs = np.array([int(d) for d in devices], dtype=np.int32)
            self.device_index = int(devs[0]) if len(devs) else 0
            res = CResult()
            self._ctx = C.c_void_p(self._lib.eth_kzg_amd_das_context_new_on_devices(
                bool(use_precomp), _vp(devs) if len(devs) else None, len(devs), float(table_budget_gb or 0.0), C.byref(res)))
            if not self._ctx.value:
                msg = C.cast(res.error_msg, C.c_char_p).value.decode() if res.error_msg else "unknown"
                self._lib.eth_kzg_free_error_message(res.error_msg)
                raise KzgError(msg)
        elif table_budget_gb is not None:
            res = CResult()
            self._ctx = C.c_void_p(self._lib.eth_kzg_amd_das_context_try_new(bool(use_precomp), self.device_index, float(table_budget_gb), C.byref(res)))
            if not self._ctx.value:
                msg = C.cast(res.error_msg, C.c_char_p).value.decode() if res.error_msg else "unknown"
                self._lib.eth_kzg_free_error_message(res.error_msg)
                raise KzgError(msg)
        elif device is None:
            self._ctx = C.c_void_p(self._lib.eth_kzg_das_context_new(bool(use_precomp)))
        else:
            self._ctx = C.c_void_p(self._lib.eth_kzg_amd_das_context_new_on_device(bool(use_precomp), int(device)))
        if not self._ctx.value:
            raise RuntimeError("eth_kzg_das_context_new returned NULL")
        if wait_tables:
            self.tables_ready(-1)

    @classmethod
    def from_trusted_setup(cls, g1_monomial, g2_monomial, *, subgroup_check=True, check_powers=False, use_precomp=True, devices=None,
                           table_budget_gb=None, wait_tables=True):
        """A context on the caller's trusted setup (eth_kzg_amd_das_context_new_with_setup; the reference's
        DASContext::new(&TrustedSetup, ..)).  g1_monomial / g2_monomial: 4096 / 65 compressed points, each list a sequence of
        48- / 96-byte strings or one flat bytes object.  subgroup_check=False is the reference's from_json_unchecked;
        check_powers=True also proves that both lists are consecutive powers of one tau over the standard generators (catches
        Lagrange points passed as monomial ones).  devices: a device list (None: what DASContext() picks).  Raises KzgError."""
        def flat(pts, size):
            if isinstance(pts, (bytes, bytearray, memoryview)):
                raw = bytes(pts)
                if len(raw) % size:
                    raise KzgError(f"InvalidSetup: {len(raw)} bytes are not a whole number of {size}-byte points")
                return raw, len(raw) // size
            pts = [bytes(x) for x in pts]
            for i, x in enumerate(pts):
                if len(x) != size:
                    raise KzgError(f"InvalidSetup: point {i} has {len(x)} bytes, not {size}")
            return b"".join(pts), len(pts)
        g1, n1 = flat(g1_monomial, 48)
        g2, n2 = flat(g2_monomial, 96)
        self = cls.__new__(cls)
        self._lib = load_library()
        self._ctx = C.c_void_p(None)
        devs = np.array([int(d) for d in devices], dtype=np.int32) if devices is not None else None
        self.device_index = int(devs[0]) if devs is not None and len(devs) else int(os.environ.get("ETH_KZG_AMD_DEVICE", "0"))
        flags = (0 if subgroup_check else SETUP_NO_SUBGROUP_CHECK) | (SETUP_CHECK_POWERS if check_powers else 0)
        res = CResult()
        b1, b2 = C.create_string_buffer(g1, max(1, len(g1))), C.create_string_buffer(g2, max(1, len(g2)))
        self._ctx = C.c_void_p(self._lib.eth_kzg_amd_das_context_new_with_setup(
            C.addressof(b1), n1, C.addressof(b2), n2, flags, bool(use_precomp), _vp(devs) if devs is not None and len(devs) else None,
            len(devs) if devs is not None else 0, float(table_budget_gb or 0.0), C.byref(res)))
        if not self._ctx.value:
            msg = C.cast(res.error_msg, C.c_char_p).value.decode() if res.error_msg else "unknown"
            self._lib.eth_kzg_free_error_message(res.error_msg)
            raise KzgError(msg)
        if wait_tables:
            self.tables_ready(-1)
        return self

    @classmethod
    def from_trusted_setup_json(cls, text_or_path, *, check_powers=True, **kwargs):
        """from_trusted_setup on the consensus-specs JSON (a JSON string, or the path of a file that holds one).  The structure
        check is ON by default here: a JSON file is where a wrong basis comes from."""
        text = text_or_path
        if not str(text_or_path).lstrip().startswith("{"):
            with open(text_or_path) as f:
                text = f.read()
        g1, g2 = parse_trusted_setup_json(text)
        return cls.from_trusted_setup(g1, g2, check_powers=check_powers, **kwargs)

    @property
    def setup_digest(self):
        """SHA-256 over the context's g1_monomial | g2_monomial bytes (eth_kzg_amd_setup_digest): which setup it holds."""
        out = C.create_string_buffer(32)
        self._lib.eth_kzg_amd_setup_digest(self._ctx, out)
        return out.raw

    def devices(self):
        """The context's device list (eth_kzg_amd_context_devices)."""
        out = np.zeros(64, dtype=np.int32)
        n = int(self._lib.eth_kzg_amd_context_devices(self._ctx, _vp(out), 64))
        return [int(d) for d in out[:n]]

    def tables_ready(self, wait_ms=0):
        """1 = final window tables in use, 0 = still on the start tables, 2 = the wide build failed (stays on what it has)."""
        return int(self._lib.eth_kzg_amd_tables_ready(self._ctx, int(wait_ms)))

    def table_build_info(self):
        """{'hipmalloc_ms', 'longest_hipmalloc_ms', 'pieces', 'bytes'} of the window tables in use (eth_kzg_amd_table_build_info)."""
        out = (C.c_double * 4)()
        self._lib.eth_kzg_amd_table_build_info(self._ctx, out)
        return {"hipmalloc_ms": round(out[0], 1), "longest_hipmalloc_ms": round(out[1], 1), "pieces": int(out[2]), "bytes": int(out[3])}

    def table_groups_ready(self):
        """How many of the 128 MSM groups already run on the wide FK20 table under construction (128: complete / nothing being built)."""
        return int(self._lib.eth_kzg_amd_table_groups_ready(self._ctx))

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.eth_kzg_das_context_free(self._ctx)
            self._ctx = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._ctx

    def _check(self, res):
        if res.status != 0:
            msg = C.string_at(res.error_msg).decode() if res.error_msg else "error"
            self._lib.eth_kzg_free_error_message(res.error_msg)
            raise KzgError(msg)

    # ---- reference API -------------------------------------------------------------------
    def blob_to_kzg_commitment(self, blob):
        if len(blob) != BYTES_PER_BLOB:  # the reference bindings reject a wrong-length slice before the FFI call
            raise KzgError("BlobHasInvalidLength")
        out = C.create_string_buffer(48)
        self._check(self._lib.eth_kzg_blob_to_kzg_commitment(self._ctx, bytes(blob), out))
        return out.raw

    def compute_cells_and_kzg_proofs(self, blob):
        if len(blob) != BYTES_PER_BLOB:
            raise KzgError("BlobHasInvalidLength")
        cells = [C.create_string_buffer(BYTES_PER_CELL) for _ in range(CELLS_PER_EXT_BLOB)]
        proofs = [C.create_string_buffer(48) for _ in range(CELLS_PER_EXT_BLOB)]
        ca, _k1 = _ptr_array(cells)
        pa, _k2 = _ptr_array(proofs)
        self._check(self._lib.eth_kzg_compute_cells_and_kzg_proofs(self._ctx, bytes(blob), ca, pa))
        return [c.raw for c in cells], [p.raw for p in proofs]

    def compute_cells(self, blob):
        if len(blob) != BYTES_PER_BLOB:
            raise KzgError("BlobHasInvalidLength")
        cells = [C.create_string_buffer(BYTES_PER_CELL) for _ in range(CELLS_PER_EXT_BLOB)]
        ca, _k = _ptr_array(cells)
        self._check(self._lib.eth_kzg_compute_cells(self._ctx, bytes(blob), ca))
        return [c.raw for c in cells]

    def verify_cell_kzg_proof_batch(self, commitments, cell_indices, cells, proofs, leaf_transcript=False):
        """leaf_transcript=True: eth_kzg_amd_verify_cell_kzg_proof_batch_ex with ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT -- the challenge is
        hashed per cell on the GPU instead of over the whole batch on a host core (same verdicts and errors; include/c_eth_kzg.h)."""
        if any(len(c) != 48 for c in commitments) or any(len(p) != 48 for p in proofs) \
                or any(len(c) != BYTES_PER_CELL for c in cells):
            raise KzgError("InvalidLength")
        ca, _k1 = _flat_ptrs(commitments, 48)
        cla, _k2 = _flat_ptrs(cells, BYTES_PER_CELL)
        pa, _k3 = _flat_ptrs(proofs, 48)
        idx = np.array(cell_indices, dtype=np.uint64) if len(cell_indices) else np.zeros(1, np.uint64)
        ok = C.c_bool(False)
        if leaf_transcript:
            self._check(self._lib.eth_kzg_amd_verify_cell_kzg_proof_batch_ex(
                self._ctx, len(commitments), _vp(ca), len(cell_indices), _vp(idx), len(cells), _vp(cla), len(proofs), _vp(pa),
                VERIFY_LEAF_TRANSCRIPT, C.byref(ok)))
            return bool(ok.value)
        self._check(self._lib.eth_kzg_verify_cell_kzg_proof_batch(
            self._ctx, len(commitments), _vp(ca), len(cell_indices), _vp(idx), len(cells), _vp(cla), len(proofs), _vp(pa),
            C.byref(ok)))
        return bool(ok.value)

    def prepare_verify_cell_kzg_proof_batch(self, commitments, cell_indices, cells, proofs):
        """Marshal a verification batch into the C ABI's pointer tables ONCE and return a zero-argument callable that runs
        eth_kzg_verify_cell_kzg_proof_batch on them: what a C caller's loop costs, without this wrapper's copying."""
        if any(len(c) != 48 for c in commitments) or any(len(p) != 48 for p in proofs) \
                or any(len(c) != BYTES_PER_CELL for c in cells):
            raise KzgError("InvalidLength")
        ca, k1 = _flat_ptrs(commitments, 48)
        cla, k2 = _flat_ptrs(cells, BYTES_PER_CELL)
        pa, k3 = _flat_ptrs(proofs, 48)
        idx = np.array(cell_indices, dtype=np.uint64) if len(cell_indices) else np.zeros(1, np.uint64)
        n = (len(commitments), len(cell_indices), len(cells), len(proofs))

        def run(_keep=(k1, k2, k3)):
            ok = C.c_bool(False)
            self._check(self._lib.eth_kzg_verify_cell_kzg_proof_batch(
                self._ctx, n[0], _vp(ca), n[1], _vp(idx), n[2], _vp(cla), n[3], _vp(pa), C.byref(ok)))
            return bool(ok.value)
        return run

    def prepare_verify_cell_kzg_proof_batch_many(self, problems, leaf_transcript=False):
        """problems = [(commitments, cell_indices, cells, proofs), ...]: marshal them into the pointer tables of
        eth_kzg_amd_verify_cell_kzg_proof_batch_many ONCE and return a zero-argument callable that runs the call and
        returns (verified list[bool], status list[int]) -- status 0 ok, 1 bad field element, 2 bad G1 point, 3 invalid
        lengths / indices: what the single form raises as KzgError.  leaf_transcript=True: eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex
        with ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT -- every problem's challenge is hashed per cell on the GPU (same verdicts and statuses)."""
        nb, lens, tabs, keep = self._marshal_many(problems)
        ver = (C.c_bool * max(1, nb))()
        st = (C.c_int32 * max(1, nb))()

        def run(_keep=keep):
            if leaf_transcript:
                self._check(self._lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex(
                    self._ctx, nb, _vp(lens[0]), _vp(tabs[0]), _vp(lens[1]), _vp(tabs[1]), _vp(lens[2]), _vp(tabs[2]), _vp(lens[3]), _vp(tabs[3]),
                    VERIFY_LEAF_TRANSCRIPT, ver, st))
            else:
                self._check(self._lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many(
                    self._ctx, nb, _vp(lens[0]), _vp(tabs[0]), _vp(lens[1]), _vp(tabs[1]), _vp(lens[2]), _vp(tabs[2]), _vp(lens[3]), _vp(tabs[3]),
                    ver, st))
            return [bool(v) for v in ver][:nb], list(st)[:nb]
        return run

    @staticmethod
    def _marshal_many(problems):
        """-> (count, lens[4][count], tabs[4][count], keep-alive): the length and pointer tables of the many-verification's arguments, in
        the order commitments, cell indices, cells, proofs"""
        nb = len(problems)
        keep, lens = [], np.zeros((4, max(1, nb)), dtype=np.uint64)
        tabs = [np.zeros(max(1, nb), dtype=np.uint64) for _ in range(4)]  # per problem: commitments**, indices*, cells**, proofs**
        for b, (commitments, cell_indices, cells, proofs) in enumerate(problems):
            if any(len(c) != 48 for c in commitments) or any(len(p) != 48 for p in proofs) \
                    or any(len(c) != BYTES_PER_CELL for c in cells):
                # a wrong byte length cannot cross the C ABI (fixed-size buffers carry no length): the single form raises
                # InvalidLength before the call; here the problem goes in with inconsistent lengths and comes back status 3
                commitments, cell_indices, cells, proofs = [], [0], [], []
            ca, k1 = _flat_ptrs(commitments, 48)
            cla, k2 = _flat_ptrs(cells, BYTES_PER_CELL)
            pa, k3 = _flat_ptrs(proofs, 48)
            idx = np.array(cell_indices, dtype=np.uint64) if len(cell_indices) else np.zeros(1, np.uint64)
            keep += [ca, k1, cla, k2, pa, k3, idx]
            lens[:, b] = (len(commitments), len(cell_indices), len(cells), len(proofs))
            tabs[0][b], tabs[1][b], tabs[2][b], tabs[3][b] = ca.ctypes.data, idx.ctypes.data, cla.ctypes.data, pa.ctypes.data
        return nb, np.ascontiguousarray(lens), tabs, keep

    def verify_cell_kzg_proof_batch_many(self, problems, leaf_transcript=False):
        """Many independent verify_cell_kzg_proof_batch problems in one call (see prepare_verify_cell_kzg_proof_batch_many)."""
        return self.prepare_verify_cell_kzg_proof_batch_many(problems, leaf_transcript)()

    def verify_cell_kzg_proof_batch_many_device(self, cell_starts, d_commitments, d_cell_indices, d_cells, d_proofs, stream=None,
                                                leaf_transcript=False):
        """The many-verification on flat arrays in device memory (eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex): cell_starts is a
        host sequence of n_batches + 1 non-decreasing entries starting at 0, problem b the entries [cell_starts[b], cell_starts[b + 1]) of
        the four arrays (integer device addresses: N*48 commitment bytes, one per cell; N uint64 indices; N*2048 cell bytes; N*48 proof
        bytes).  -> (verified list[bool], status list[int]).  leaf_transcript=True: neither cells nor proofs are copied to the host;
        False: the reference's challenges, for which they are (the slow way)."""
        cs = np.ascontiguousarray(np.array(cell_starts, dtype=np.uint64))
        nb = max(0, len(cs) - 1)
        ver = (C.c_bool * max(1, nb))()
        st = (C.c_int32 * max(1, nb))()
        self._check(self._lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex(
            self._ctx, nb, _vp(cs) if len(cs) else None, C.c_void_p(d_commitments), C.c_void_p(d_cell_indices), C.c_void_p(d_cells),
            C.c_void_p(d_proofs), VERIFY_LEAF_TRANSCRIPT if leaf_transcript else 0, ver, st, C.c_void_p(stream) if stream else None))
        return [bool(v) for v in ver][:nb], list(st)[:nb]

    @staticmethod
    def _marshal_columns(commitments, column_indices, cells, proofs):
        """-> (n_blobs, n_columns, commitments**, indices*, cells***, proofs***, keep-alive): the arguments of eth_kzg_amd_verify_data_columns
        (cells[j][i] / proofs[j][i]: blob i in column j)"""
        nb, nc = len(commitments), len(column_indices)
        if len(cells) != nc or len(proofs) != nc or any(len(c) != nb for c in cells) or any(len(p) != nb for p in proofs) \
                or any(len(c) != 48 for c in commitments) or any(len(p) != 48 for col in proofs for p in col) \
                or any(len(c) != BYTES_PER_CELL for col in cells for c in col):
            raise KzgError("InvalidLength")  # (fixed-size buffers carry no length across the C ABI)
        ca, k1 = _flat_ptrs(commitments, 48)
        idx = np.array(column_indices, dtype=np.uint64) if nc else np.zeros(1, np.uint64)
        keep, tabs = [k1], [np.zeros(max(1, nc), dtype=np.uint64) for _ in range(2)]
        for j in range(nc):
            cla, k2 = _flat_ptrs(cells[j], BYTES_PER_CELL)
            pa, k3 = _flat_ptrs(proofs[j], 48)
            keep += [cla, k2, pa, k3]
            tabs[0][j], tabs[1][j] = cla.ctypes.data, pa.ctypes.data
        return nb, nc, ca, idx, tabs[0], tabs[1], keep

    def verify_data_columns(self, commitments, column_indices, cells, proofs, leaf_transcript=False):
        """The data columns of one block, the block's commitments given once (eth_kzg_amd_verify_data_columns): commitments[i] of blob i,
        column j = (column_indices[j], cells[j][i], proofs[j][i]).  -> (verified list[bool], status list[int]) per column, exactly what
        verify_cell_kzg_proof_batch_many gives the column as a problem of its own."""
        nb, nc, ca, idx, cla, pa, _keep = self._marshal_columns(commitments, column_indices, cells, proofs)
        ver = (C.c_bool * max(1, nc))()
        st = (C.c_int32 * max(1, nc))()
        self._check(self._lib.eth_kzg_amd_verify_data_columns(self._ctx, nb, _vp(ca), nc, _vp(idx), _vp(cla), _vp(pa),
                                                              VERIFY_LEAF_TRANSCRIPT if leaf_transcript else 0, ver, st))
        return [bool(v) for v in ver][:nc], list(st)[:nc]

    def verify_data_columns_device(self, n_blobs, d_commitments, column_indices, d_cells, d_proofs, stream=None, leaf_transcript=False):
        """The same on arrays in device memory (eth_kzg_amd_verify_data_columns_device; integer device addresses): d_commitments
        n_blobs*48 bytes, d_cells [columns][n_blobs][2048], d_proofs [columns][n_blobs][48]; column_indices a host sequence.
        leaf_transcript=True: neither cells nor proofs are copied to the host."""
        idx = np.ascontiguousarray(np.array(column_indices, dtype=np.uint64)) if len(column_indices) else np.zeros(1, np.uint64)
        nc = len(column_indices)
        ver = (C.c_bool * max(1, nc))()
        st = (C.c_int32 * max(1, nc))()
        self._check(self._lib.eth_kzg_amd_verify_data_columns_device(
            self._ctx, n_blobs, C.c_void_p(d_commitments), nc, _vp(idx), C.c_void_p(d_cells), C.c_void_p(d_proofs),
            VERIFY_LEAF_TRANSCRIPT if leaf_transcript else 0, ver, st, C.c_void_p(stream) if stream else None))
        return [bool(v) for v in ver][:nc], list(st)[:nc]

    # ---- partial data columns: present[j] is a Python int, bit i = blob i (so that stray bits can be expressed)
    @staticmethod
    def _present_words(n_blobs, present):
        """-> uint64 [n_columns][W], W = ceil(n_blobs / 64): the bitmaps as the C ABI takes them; bits beyond 64 W cannot cross it"""
        words = (n_blobs + 63) // 64
        if any(p < 0 or p >> (64 * words) for p in present):
            raise KzgError("InvalidLength")
        out = np.zeros((max(1, len(present)), max(1, words)), dtype=np.uint64)
        for j, p in enumerate(present):
            for w in range(words):
                out[j, w] = (p >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
        return out, words

    @classmethod
    def _marshal_partial_columns(cls, commitments, column_indices, present, cells, proofs):
        """-> (n_blobs, n_columns, commitments**, indices*, present**, cells***, proofs***, keep-alive): the arguments of
        eth_kzg_amd_verify_partial_data_columns (cells[j][k] / proofs[j][k]: the k-th set bit of present[j])"""
        nb, nc = len(commitments), len(column_indices)
        if len(present) != nc or len(cells) != nc or len(proofs) != nc or any(len(c) != 48 for c in commitments) \
                or any(len(cells[j]) != len(proofs[j]) for j in range(nc)) or any(len(p) != 48 for col in proofs for p in col) \
                or any(len(c) != BYTES_PER_CELL for col in cells for c in col):
            raise KzgError("InvalidLength")  # (fixed-size buffers carry no length across the C ABI)
        bits, _words = cls._present_words(nb, present)
        if any(len(cells[j]) != bin(present[j] & ((1 << nb) - 1)).count("1") for j in range(nc)):
            raise KzgError("InvalidLength")  # (a column's lists are as long as its bitmap says: m_j, the set bits below n_blobs)
        ca, k1 = _flat_ptrs(commitments, 48)
        idx = np.array(column_indices, dtype=np.uint64) if nc else np.zeros(1, np.uint64)
        keep, tabs = [k1, bits], [np.zeros(max(1, nc), dtype=np.uint64) for _ in range(3)]
        for j in range(nc):
            cla, k2 = _flat_ptrs(cells[j], BYTES_PER_CELL)
            pa, k3 = _flat_ptrs(proofs[j], 48)
            keep += [cla, k2, pa, k3]
            tabs[0][j], tabs[1][j], tabs[2][j] = bits[j].ctypes.data, cla.ctypes.data, pa.ctypes.data
        return nb, nc, ca, idx, tabs[0], tabs[1], tabs[2], keep

    def verify_partial_data_columns(self, commitments, column_indices, present, cells, proofs, leaf_transcript=False):
        """Partial data columns of one block (eth_kzg_amd_verify_partial_data_columns): commitments[i] of every blob i of the block,
        column j = (column_indices[j], present[j], cells[j][k], proofs[j][k]) with k over the set bits of present[j] in ascending blob
        order.  -> (verified list[bool], status list[int]) per column, exactly what verify_cell_kzg_proof_batch_many gives the column's
        present cells as a problem of its own."""
        nb, nc, ca, idx, ba, cla, pa, _keep = self._marshal_partial_columns(commitments, column_indices, present, cells, proofs)
        ver = (C.c_bool * max(1, nc))()
        st = (C.c_int32 * max(1, nc))()
        self._check(self._lib.eth_kzg_amd_verify_partial_data_columns(self._ctx, nb, _vp(ca), nc, _vp(idx), _vp(ba), _vp(cla), _vp(pa),
                                                                      VERIFY_LEAF_TRANSCRIPT if leaf_transcript else 0, ver, st))
        return [bool(v) for v in ver][:nc], list(st)[:nc]

    def verify_partial_data_columns_device(self, n_blobs, d_commitments, column_indices, present, d_cells, d_proofs, stream=None,
                                           leaf_transcript=False):
        """The same on arrays in device memory (eth_kzg_amd_verify_partial_data_columns_device; integer device addresses): d_commitments
        n_blobs*48 bytes; d_cells [N][2048] and d_proofs [N][48] packed column after column, within a column in ascending blob order, a
        column taking as many entries as its bitmap has set bits; column_indices and present host sequences."""
        nc = len(column_indices)
        if len(present) != nc:
            raise KzgError("InvalidLength")
        idx = np.ascontiguousarray(np.array(column_indices, dtype=np.uint64)) if nc else np.zeros(1, np.uint64)
        bits, _words = self._present_words(n_blobs, present)
        ver = (C.c_bool * max(1, nc))()
        st = (C.c_int32 * max(1, nc))()
        self._check(self._lib.eth_kzg_amd_verify_partial_data_columns_device(
            self._ctx, n_blobs, C.c_void_p(d_commitments), nc, _vp(idx), _vp(bits), C.c_void_p(d_cells), C.c_void_p(d_proofs),
            VERIFY_LEAF_TRANSCRIPT if leaf_transcript else 0, ver, st, C.c_void_p(stream) if stream else None))
        return [bool(v) for v in ver][:nc], list(st)[:nc]

    # ---- a block's data columns computed and recovered in column layout (cells[c][i] / proofs[c][i]: blob i in column c)
    def compute_data_columns(self, blobs, want_commitments=True, want_cells=True, want_proofs=True, prefill=0):
        """The proposer's call (eth_kzg_amd_compute_data_columns): blobs -> (status list, commitments[i], cells[c][i], proofs[c][i]) with
        c over the 128 columns; an output that was not asked for is None.  Byte for byte what blob_to_kzg_commitment_batch and
        compute_cells_and_kzg_proofs_batch give, transposed; the slots of a blob with status 1 come back as they were: `prefill` bytes."""
        n = len(blobs)
        if any(len(b) != BYTES_PER_BLOB for b in blobs):
            raise KzgError("InvalidLength")
        ba, _kb = _flat_ptrs(blobs, BYTES_PER_BLOB)
        comm, ci, _co = _out_ptrs(1, n, 48)
        cells, _ci, cpp = _out_ptrs(CELLS_PER_EXT_BLOB, n, BYTES_PER_CELL)
        proofs, _pi, ppp = _out_ptrs(CELLS_PER_EXT_BLOB, n, 48)
        for out in (comm, cells, proofs):
            out.fill(prefill)
        st = (C.c_int32 * max(1, n))()
        self._check(self._lib.eth_kzg_amd_compute_data_columns(
            self._ctx, n, _vp(ba) if n else None, _vp(ci) if want_commitments else None, _vp(cpp) if want_cells else None,
            _vp(ppp) if want_proofs else None, st))
        return (list(st)[:n], _split(comm, 1, n, 48)[0] if want_commitments else None,
                _split(cells, CELLS_PER_EXT_BLOB, n, BYTES_PER_CELL) if want_cells else None,
                _split(proofs, CELLS_PER_EXT_BLOB, n, 48) if want_proofs else None)

    def compute_data_columns_device(self, n_blobs, d_blobs, d_commitments, d_cells, d_proofs, want_status=True, stream=None):
        """The same on flat buffers in device memory (eth_kzg_amd_compute_data_columns_device; integer device addresses): d_commitments
        n_blobs*48, d_cells [128][n_blobs][2048], d_proofs [128][n_blobs][48], each may be 0 / None.  want_status=False with a stream:
        returns without synchronising."""
        st = (C.c_int32 * max(1, n_blobs))() if want_status else None
        self._check(self._lib.eth_kzg_amd_compute_data_columns_device(
            self._ctx, n_blobs, C.c_void_p(d_blobs) if d_blobs else None, C.c_void_p(d_commitments) if d_commitments else None,
            C.c_void_p(d_cells) if d_cells else None, C.c_void_p(d_proofs) if d_proofs else None, st, C.c_void_p(stream) if stream else None))
        return list(st)[:n_blobs] if want_status else None

    def blobs_to_data_columns(self, items, verify=False, want_cells=True, want_proofs=True, prefill=0):
        """The call of a node that HOLDS the cell proofs (eth_kzg_amd_blobs_to_data_columns): items = [(blob, commitment, [128 cell
        proofs]), ...] -> (verified list[bool] or None, status list, cells[c][i], proofs[c][i]) with c over the 128 columns; an output
        that was not asked for is None.  verify=False: the commitment may be None (it is not read), status is compute_data_columns'
        and proofs[c][i] is items[i][2][c] byte for byte.  verify=True (ETH_KZG_AMD_COLUMNS_VERIFY_PROOFS): verified and status are
        verify_blob_cell_proofs_many's.  The slots of an item that is refused or fails come back as they were: `prefill` bytes."""
        n = len(items)
        if not verify:
            items = [(b, c if c is not None else bytes(48), ps) for b, c, ps in items]
        ba, ca, pa, keep = DASContext._marshal_blob_cell_proofs(items)
        cells, _ci, cpp = _out_ptrs(CELLS_PER_EXT_BLOB, n, BYTES_PER_CELL) if want_cells else (None, None, None)
        proofs, _pi, ppp = _out_ptrs(CELLS_PER_EXT_BLOB, n, 48) if want_proofs else (None, None, None)
        for out in (cells, proofs):
            if out is not None:
                out.fill(prefill)
        ver = (C.c_bool * max(1, n))()
        st = (C.c_int32 * max(1, n))()
        self._check(self._lib.eth_kzg_amd_blobs_to_data_columns(
            self._ctx, n, _vp(ba) if n else None, _vp(ca) if verify else None, _vp(pa) if n else None,
            COLUMNS_VERIFY_PROOFS if verify else 0, _vp(cpp) if want_cells else None, _vp(ppp) if want_proofs else None,
            ver if verify else None, st))
        del keep
        return ([bool(v) for v in ver][:n] if verify else None, list(st)[:n],
                _split(cells, CELLS_PER_EXT_BLOB, n, BYTES_PER_CELL) if want_cells else None,
                _split(proofs, CELLS_PER_EXT_BLOB, n, 48) if want_proofs else None)

    def blobs_to_data_columns_device(self, n_blobs, d_blobs, d_commitments, d_proofs, d_out_cells, d_out_proofs, verify=False, want_status=True,
                                     stream=None):
        """The same on flat buffers in device memory (eth_kzg_amd_blobs_to_data_columns_device; integer device addresses): d_blobs
        n_blobs*131072 (4-byte aligned), d_commitments n_blobs*48, d_proofs [n_blobs][128][48], d_out_cells [128][n_blobs][2048] (4-byte
        aligned), d_out_proofs [128][n_blobs][48]; the outputs, and without verify the commitments, may be 0 / None.
        -> (verified list[bool] or None, status list or None).  verify=False, want_status=False and a stream: returns without
        synchronising."""
        p = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        ver = (C.c_bool * max(1, n_blobs))() if verify else None
        st = (C.c_int32 * max(1, n_blobs))() if want_status or verify else None
        self._check(self._lib.eth_kzg_amd_blobs_to_data_columns_device(
            self._ctx, n_blobs, p(d_blobs), p(d_commitments), p(d_proofs), COLUMNS_VERIFY_PROOFS if verify else 0, p(d_out_cells), p(d_out_proofs),
            ver, st, p(stream)))
        return [bool(v) for v in ver][:n_blobs] if verify else None, list(st)[:n_blobs] if st is not None else None

    def test_blob_to_columns(self, blobs, n_total=None, b0=0, blob_half=True, guard=0xA5):
        """eth_kzg_amd_test_blob_to_columns (hooks library): the kernel alone over a matrix of n_total blobs filled with `guard`
        -> (matrix [128][n_total] of cell bytes, bad[n])"""
        n = len(blobs)
        n_total = n if n_total is None else n_total
        if any(len(b) != BYTES_PER_BLOB for b in blobs):
            raise KzgError("InvalidLength")
        ba, keep = _alias_ptrs(list(blobs))
        m = np.full(CELLS_PER_EXT_BLOB * max(1, n_total) * BYTES_PER_CELL, guard, dtype=np.uint8)
        bad = (C.c_int32 * max(1, n))()
        rc = self._lib.eth_kzg_amd_test_blob_to_columns(self._ctx, n, _vp(ba), n_total, b0, 1 if blob_half else 0, _vp(m), bad)
        if rc != 0:
            raise KzgError("test_blob_to_columns: status %d" % rc)
        del keep
        return _split(m, CELLS_PER_EXT_BLOB, n_total, BYTES_PER_CELL), list(bad)[:n]

    def recover_data_columns(self, column_indices, cells, want_cells=True, want_proofs=True, prefill=0):
        """The supernode's call (eth_kzg_amd_recover_data_columns): column_indices[j] and cells[j][i] (blob i in the j-th column given)
        -> (status list per blob, cells[c][i], proofs[c][i]) over all 128 columns; exactly recover_cells_and_kzg_proofs_batch per blob.
        The slots of a blob whose status is not 0 come back as they were: `prefill` bytes."""
        nc = len(column_indices)
        nb = len(cells[0]) if nc else 0
        if len(cells) != nc or any(len(col) != nb for col in cells) or any(len(c) != BYTES_PER_CELL for col in cells for c in col):
            raise KzgError("InvalidLength")
        idx = np.array(column_indices, dtype=np.uint64) if nc else np.zeros(1, np.uint64)
        keep, tab = [], np.zeros(max(1, nc), dtype=np.uint64)
        for j in range(nc):
            cla, k = _flat_ptrs(cells[j], BYTES_PER_CELL)
            keep += [cla, k]
            tab[j] = cla.ctypes.data
        out_cells, _ci, ocp = _out_ptrs(CELLS_PER_EXT_BLOB, nb, BYTES_PER_CELL)
        out_proofs, _pi, opp = _out_ptrs(CELLS_PER_EXT_BLOB, nb, 48)
        out_cells.fill(prefill)
        out_proofs.fill(prefill)
        st = (C.c_int32 * max(1, nb))()
        self._check(self._lib.eth_kzg_amd_recover_data_columns(self._ctx, nb, nc, _vp(idx), _vp(tab), _vp(ocp) if want_cells else None,
                                                               _vp(opp) if want_proofs else None, st))
        return (list(st)[:nb], _split(out_cells, CELLS_PER_EXT_BLOB, nb, BYTES_PER_CELL) if want_cells else None,
                _split(out_proofs, CELLS_PER_EXT_BLOB, nb, 48) if want_proofs else None)

    def recover_data_columns_device(self, n_blobs, column_indices, d_cells, d_out_cells, d_out_proofs, stream=None):
        """The same on device memory (eth_kzg_amd_recover_data_columns_device): d_cells [len(column_indices)][n_blobs][2048],
        d_out_cells [128][n_blobs][2048], d_out_proofs [128][n_blobs][48] (either may be 0 / None).  -> the per-blob status list."""
        nc = len(column_indices)
        idx = np.ascontiguousarray(np.array(column_indices, dtype=np.uint64)) if nc else np.zeros(1, np.uint64)
        st = (C.c_int32 * max(1, n_blobs))()
        self._check(self._lib.eth_kzg_amd_recover_data_columns_device(
            self._ctx, n_blobs, nc, _vp(idx), C.c_void_p(d_cells) if d_cells else None, C.c_void_p(d_out_cells) if d_out_cells else None,
            C.c_void_p(d_out_proofs) if d_out_proofs else None, st, C.c_void_p(stream) if stream else None))
        return list(st)[:n_blobs]

    def recover_data_columns_checked(self, column_indices, cells, commitments=None, want_blobs=True, want_commitments=True, want_cells=True,
                                     want_proofs=True, prefill=0):
        """The recovery checked against the block's commitments (eth_kzg_amd_recover_data_columns_checked): column_indices[j], cells[j][i]
        and commitments[i] (None: nothing is compared) -> (status list per blob, blobs[i], commitments[i], cells[c][i], proofs[c][i]); an
        output that was not asked for is None.  Status 6: the recovered polynomial's commitment differs from commitments[i], compared
        on bytes.  The slots of a blob whose status is not 0 come back as they were: `prefill` bytes."""
        nc = len(column_indices)
        nb = len(cells[0]) if nc else 0
        if len(cells) != nc or any(len(col) != nb for col in cells) or any(len(c) != BYTES_PER_CELL for col in cells for c in col):
            raise KzgError("InvalidLength")
        if commitments is not None and (len(commitments) != nb or any(len(c) != 48 for c in commitments)):
            raise KzgError("InvalidLength")  # (fixed-size buffers carry no length across the C ABI)
        idx = np.array(column_indices, dtype=np.uint64) if nc else np.zeros(1, np.uint64)
        keep, tab = [], np.zeros(max(1, nc), dtype=np.uint64)
        for j in range(nc):
            cla, k = _flat_ptrs(cells[j], BYTES_PER_CELL)
            keep += [cla, k]
            tab[j] = cla.ctypes.data
        ca, _kc = _flat_ptrs(commitments, 48) if commitments is not None else (None, None)
        out_blobs, bi, _bo = _out_ptrs(1, nb, BYTES_PER_BLOB)
        out_comm, ki, _ko = _out_ptrs(1, nb, 48)
        out_cells, _ci, ocp = _out_ptrs(CELLS_PER_EXT_BLOB, nb, BYTES_PER_CELL)
        out_proofs, _pi, opp = _out_ptrs(CELLS_PER_EXT_BLOB, nb, 48)
        for out in (out_blobs, out_comm, out_cells, out_proofs):
            out.fill(prefill)
        st = (C.c_int32 * max(1, nb))()
        self._check(self._lib.eth_kzg_amd_recover_data_columns_checked(
            self._ctx, nb, _vp(ca) if ca is not None else None, nc, _vp(idx), _vp(tab), _vp(bi) if want_blobs else None,
            _vp(ki) if want_commitments else None, _vp(ocp) if want_cells else None, _vp(opp) if want_proofs else None, st))
        return (list(st)[:nb], _split(out_blobs, 1, nb, BYTES_PER_BLOB)[0] if want_blobs else None,
                _split(out_comm, 1, nb, 48)[0] if want_commitments else None,
                _split(out_cells, CELLS_PER_EXT_BLOB, nb, BYTES_PER_CELL) if want_cells else None,
                _split(out_proofs, CELLS_PER_EXT_BLOB, nb, 48) if want_proofs else None)

    def recover_data_columns_checked_device(self, n_blobs, column_indices, d_cells, d_commitments=None, d_out_blobs=None, d_out_commitments=None,
                                            d_out_cells=None, d_out_proofs=None, stream=None):
        """The same on device memory (eth_kzg_amd_recover_data_columns_checked_device; integer device addresses, each of the five behind
        d_cells may be 0 / None): d_cells [len(column_indices)][n_blobs][2048], d_commitments and d_out_commitments n_blobs*48,
        d_out_blobs [n_blobs][131072], d_out_cells [128][n_blobs][2048], d_out_proofs [128][n_blobs][48].  -> the per-blob status list."""
        nc = len(column_indices)
        idx = np.ascontiguousarray(np.array(column_indices, dtype=np.uint64)) if nc else np.zeros(1, np.uint64)
        st = (C.c_int32 * max(1, n_blobs))()
        vp = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        self._check(self._lib.eth_kzg_amd_recover_data_columns_checked_device(
            self._ctx, n_blobs, vp(d_commitments), nc, _vp(idx), vp(d_cells), vp(d_out_blobs), vp(d_out_commitments), vp(d_out_cells),
            vp(d_out_proofs), st, vp(stream)))
        return list(st)[:n_blobs]

    def verify_cell_kzg_proof_batch_partial(self, commitments, cell_indices, cells, proofs, shard_begin, shard_end):
        """This rank's share of a sharded verification: the whole batch goes in (the challenge hashes all of it), the
        cells [shard_begin, shard_end) are evaluated, 96 bytes come back (sharding.verify_cell_kzg_proof_batch_sharded)."""
        if any(len(c) != 48 for c in commitments) or any(len(p) != 48 for p in proofs) \
                or any(len(c) != BYTES_PER_CELL for c in cells):
            raise KzgError("InvalidLength")
        ca, _k1 = _flat_ptrs(commitments, 48)
        cla, _k2 = _flat_ptrs(cells, BYTES_PER_CELL)
        pa, _k3 = _flat_ptrs(proofs, 48)
        idx = np.array(cell_indices, dtype=np.uint64) if len(cell_indices) else np.zeros(1, np.uint64)
        out = C.create_string_buffer(VERIFY_PARTIAL_BYTES)
        self._check(self._lib.eth_kzg_amd_verify_cell_kzg_proof_batch_partial(
            self._ctx, len(commitments), _vp(ca), len(cell_indices), _vp(idx), len(cells), _vp(cla), len(proofs), _vp(pa),
            int(shard_begin), int(shard_end), out))
        return out.raw

    def verify_cell_kzg_proof_batch_combine(self, partials):
        """Add the gathered 96-byte partials of all ranks and run the pairing check."""
        blob = b"".join(partials)
        if len(blob) % VERIFY_PARTIAL_BYTES:
            raise KzgError("InvalidLength")
        ok = C.c_bool(False)
        self._check(self._lib.eth_kzg_amd_verify_cell_kzg_proof_batch_combine(
            self._ctx, len(blob) // VERIFY_PARTIAL_BYTES, blob, C.byref(ok)))
        return bool(ok.value)

    def recover_cells_and_kzg_proofs(self, cell_indices, cells):
        if any(len(c) != BYTES_PER_CELL for c in cells):
            raise KzgError("InvalidLength")
        cla, _k = _ptr_array(cells)
        idx = (C.c_uint64 * max(1, len(cell_indices)))(*cell_indices)
        out_cells = [C.create_string_buffer(BYTES_PER_CELL) for _ in range(CELLS_PER_EXT_BLOB)]
        out_proofs = [C.create_string_buffer(48) for _ in range(CELLS_PER_EXT_BLOB)]
        oca, _k1 = _ptr_array(out_cells)
        opa, _k2 = _ptr_array(out_proofs)
        self._check(self._lib.eth_kzg_recover_cells_and_proofs(
            self._ctx, len(cells), cla, len(cell_indices), idx, oca, opa))
        return [c.raw for c in out_cells], [p.raw for p in out_proofs]

    # ---- EIP-4844 single-point operations (crates/eip4844/src/{prover,verifier}.rs) ----
    def compute_kzg_proof(self, blob, z):
        if len(blob) != BYTES_PER_BLOB or len(z) != 32:
            raise KzgError("InvalidLength")
        proof, y = C.create_string_buffer(48), C.create_string_buffer(32)
        self._check(self._lib.eth_kzg_compute_kzg_proof(self._ctx, bytes(blob), bytes(z), proof, y))
        return proof.raw, y.raw

    def compute_blob_kzg_proof(self, blob, commitment):
        if len(blob) != BYTES_PER_BLOB or len(commitment) != 48:
            raise KzgError("InvalidLength")
        proof = C.create_string_buffer(48)
        self._check(self._lib.eth_kzg_compute_blob_kzg_proof(self._ctx, bytes(blob), bytes(commitment), proof))
        return proof.raw

    def verify_kzg_proof(self, commitment, z, y, proof):
        if len(commitment) != 48 or len(proof) != 48 or len(z) != 32 or len(y) != 32:
            raise KzgError("InvalidLength")
        ok = C.c_bool(False)
        self._check(self._lib.eth_kzg_verify_kzg_proof(self._ctx, bytes(commitment), bytes(z), bytes(y), bytes(proof), C.byref(ok)))
        return bool(ok.value)

    def prepare_verify_kzg_proof_many(self, items):
        """items = [(commitment, z, y, proof), ...]: marshal them into the pointer tables of eth_kzg_amd_verify_kzg_proof_many ONCE and
        return a zero-argument callable that runs the call and returns (verified list[bool], status list[int]) -- per item what
        verify_kzg_proof says of it alone: status 2 a bad G1 point, else 1 z or y >= r (what the single form raises as KzgError), else 0
        and the verdict.  A wrong byte length cannot cross the C ABI and raises InvalidLength here."""
        n = len(items)
        if any(len(c) != 48 or len(z) != 32 or len(y) != 32 or len(p) != 48 for c, z, y, p in items):
            raise KzgError("InvalidLength")
        ca, k1 = _flat_ptrs([it[0] for it in items], 48)
        za, k2 = _flat_ptrs([it[1] for it in items], 32)
        ya, k3 = _flat_ptrs([it[2] for it in items], 32)
        pa, k4 = _flat_ptrs([it[3] for it in items], 48)
        ver = (C.c_bool * max(1, n))()
        st = (C.c_int32 * max(1, n))()

        def run(_keep=(k1, k2, k3, k4)):
            self._check(self._lib.eth_kzg_amd_verify_kzg_proof_many(self._ctx, n, _vp(ca), _vp(za), _vp(ya), _vp(pa), ver, st))
            return [bool(v) for v in ver][:n], list(st)[:n]
        return run

    def verify_kzg_proof_many(self, items):
        """Many verify_kzg_proof items in one call, a verdict for each (see prepare_verify_kzg_proof_many)."""
        return self.prepare_verify_kzg_proof_many(items)()

    def verify_kzg_proof_many_device(self, n, d_commitments, d_zs, d_ys, d_proofs, stream=None):
        """The same on flat arrays in device memory (eth_kzg_amd_verify_kzg_proof_many_device): integer device addresses of n*48
        commitment bytes, n*32 z and y bytes (big-endian, 4-byte aligned) and n*48 proof bytes.  -> (verified list[bool], status
        list[int]).  Synchronous; waits for what `stream` (None: the default stream) has queued.  The leaves are hashed on the GPU."""
        ver = (C.c_bool * max(1, n))()
        st = (C.c_int32 * max(1, n))()
        self._check(self._lib.eth_kzg_amd_verify_kzg_proof_many_device(
            self._ctx, n, C.c_void_p(d_commitments), C.c_void_p(d_zs), C.c_void_p(d_ys), C.c_void_p(d_proofs), ver, st,
            C.c_void_p(stream) if stream else None))
        return [bool(v) for v in ver][:n], list(st)[:n]

    def prepare_verify_blob_kzg_proof_many(self, items):
        """items = [(blob, commitment, proof), ...]: marshal them into the pointer tables of eth_kzg_amd_verify_blob_kzg_proof_many ONCE
        (a blob object named several times is not copied) and return a zero-argument callable that runs the call and returns (verified
        list[bool], status list[int]) -- per item what verify_blob_kzg_proof says of it alone: status 1 the blob holds an element >= r,
        else 2 a bad G1 point (what the single form raises as KzgError), else 0 and the verdict.  A wrong byte length cannot cross the C
        ABI and raises InvalidLength here."""
        n = len(items)
        if any(len(b) != BYTES_PER_BLOB or len(c) != 48 or len(p) != 48 for b, c, p in items):
            raise KzgError("InvalidLength")
        ba, k1 = _alias_ptrs([it[0] for it in items])
        ca, k2 = _flat_ptrs([it[1] for it in items], 48)
        pa, k3 = _flat_ptrs([it[2] for it in items], 48)
        ver = (C.c_bool * max(1, n))()
        st = (C.c_int32 * max(1, n))()

        def run(_keep=(k1, k2, k3)):
            self._check(self._lib.eth_kzg_amd_verify_blob_kzg_proof_many(self._ctx, n, _vp(ba), _vp(ca), _vp(pa), ver, st))
            return [bool(v) for v in ver][:n], list(st)[:n]
        return run

    def verify_blob_kzg_proof_many(self, items):
        """Many verify_blob_kzg_proof items in one call, a verdict for each (see prepare_verify_blob_kzg_proof_many)."""
        return self.prepare_verify_blob_kzg_proof_many(items)()

    def verify_blob_kzg_proof_many_device(self, n, d_blobs, d_commitments, d_proofs, stream=None):
        """The same on flat arrays in device memory (eth_kzg_amd_verify_blob_kzg_proof_many_device): integer device addresses of
        n*131072 blob bytes (read where they lie), n*48 commitment and n*48 proof bytes.  -> (verified list[bool], status list[int]).
        Synchronous; waits for what `stream` (None: the default stream) has queued."""
        ver = (C.c_bool * max(1, n))()
        st = (C.c_int32 * max(1, n))()
        self._check(self._lib.eth_kzg_amd_verify_blob_kzg_proof_many_device(
            self._ctx, n, C.c_void_p(d_blobs), C.c_void_p(d_commitments), C.c_void_p(d_proofs), ver, st,
            C.c_void_p(stream) if stream else None))
        return [bool(v) for v in ver][:n], list(st)[:n]

    @staticmethod
    def _marshal_blob_cell_proofs(items):
        """-> (blobs**, commitments**, proofs***, keep-alive): the pointer tables of eth_kzg_amd_verify_blob_cell_proofs_many; a blob
        object named several times is not copied"""
        n = len(items)
        if any(len(b) != BYTES_PER_BLOB or len(c) != 48 or len(ps) != CELLS_PER_EXT_BLOB or any(len(p) != 48 for p in ps) for b, c, ps in items):
            raise KzgError("InvalidLength")
        ba, k1 = _alias_ptrs([it[0] for it in items])
        ca, k2 = _flat_ptrs([it[1] for it in items], 48)
        inner, k3 = _flat_ptrs([p for it in items for p in it[2]], 48)
        outer = np.uint64(inner.ctypes.data) + np.arange(max(1, n), dtype=np.uint64) * np.uint64(CELLS_PER_EXT_BLOB * 8)
        return ba, ca, outer, (k1, k2, k3, inner)

    def prepare_verify_blob_cell_proofs_many(self, items):
        """items = [(blob, commitment, [128 cell proofs]), ...]: marshal them into the pointer tables of
        eth_kzg_amd_verify_blob_cell_proofs_many ONCE and return a zero-argument callable that runs the call and returns (verified
        list[bool], status list[int]) -- per item what compute_cells + verify_cell_kzg_proof_batch([commitment] * 128, 0..127, cells,
        proofs) say of it: status 1 the blob holds an element >= r, else 2 a bad G1 point, else 0 and the verdict.  A wrong byte
        length or proof count cannot cross the C ABI and raises InvalidLength here."""
        n = len(items)
        ba, ca, pa, keep = self._marshal_blob_cell_proofs(items)
        ver = (C.c_bool * max(1, n))()
        st = (C.c_int32 * max(1, n))()

        def run(_keep=keep):
            self._check(self._lib.eth_kzg_amd_verify_blob_cell_proofs_many(self._ctx, n, _vp(ba), _vp(ca), _vp(pa), ver, st))
            return [bool(v) for v in ver][:n], list(st)[:n]
        return run

    def verify_blob_cell_proofs_many(self, items):
        """Many blobs against their 128 cell proofs in one call, a verdict for each (see prepare_verify_blob_cell_proofs_many)."""
        return self.prepare_verify_blob_cell_proofs_many(items)()

    def verify_blob_cell_proofs_many_device(self, n, d_blobs, d_commitments, d_proofs, stream=None):
        """The same on flat arrays in device memory (eth_kzg_amd_verify_blob_cell_proofs_many_device): integer device addresses of
        n*131072 blob bytes (4-byte aligned), n*48 commitment and n*128*48 proof bytes.  -> (verified list[bool], status list[int]).
        Synchronous; waits for what `stream` (None: the default stream) has queued."""
        ver = (C.c_bool * max(1, n))()
        st = (C.c_int32 * max(1, n))()
        self._check(self._lib.eth_kzg_amd_verify_blob_cell_proofs_many_device(
            self._ctx, n, C.c_void_p(d_blobs), C.c_void_p(d_commitments), C.c_void_p(d_proofs), ver, st,
            C.c_void_p(stream) if stream else None))
        return [bool(v) for v in ver][:n], list(st)[:n]

    def test_blob_extension(self, blobs):
        """eth_kzg_amd_test_blob_extension (hooks library): -> (cells[n][128] as bytes, bad[n])"""
        n = len(blobs)
        if any(len(b) != BYTES_PER_BLOB for b in blobs):
            raise KzgError("InvalidLength")
        ba, keep = _alias_ptrs(list(blobs))
        out = np.zeros(max(1, n) * CELLS_PER_EXT_BLOB * BYTES_PER_CELL, dtype=np.uint8)
        bad = (C.c_int32 * max(1, n))()
        rc = self._lib.eth_kzg_amd_test_blob_extension(self._ctx, n, _vp(ba), _vp(out), bad)
        if rc != 0:
            raise KzgError("test_blob_extension: status %d" % rc)
        raw = out.tobytes()
        cells = [[raw[(b * CELLS_PER_EXT_BLOB + k) * BYTES_PER_CELL:(b * CELLS_PER_EXT_BLOB + k + 1) * BYTES_PER_CELL] for k in range(CELLS_PER_EXT_BLOB)]
                 for b in range(n)]
        del keep
        return cells, list(bad)[:n]

    def verify_blob_kzg_proof(self, blob, commitment, proof):
        if len(blob) != BYTES_PER_BLOB or len(commitment) != 48 or len(proof) != 48:
            raise KzgError("InvalidLength")
        ok = C.c_bool(False)
        self._check(self._lib.eth_kzg_verify_blob_kzg_proof(self._ctx, bytes(blob), bytes(commitment), bytes(proof), C.byref(ok)))
        return bool(ok.value)

    def verify_blob_kzg_proof_batch(self, blobs, commitments, proofs):
        if any(len(b) != BYTES_PER_BLOB for b in blobs) or any(len(c) != 48 for c in commitments) \
                or any(len(p) != 48 for p in proofs):
            raise KzgError("InvalidLength")
        ba, _k1 = _ptr_array(blobs)
        ca, _k2 = _ptr_array(commitments)
        pa, _k3 = _ptr_array(proofs)
        ok = C.c_bool(False)
        self._check(self._lib.eth_kzg_verify_blob_kzg_proof_batch(self._ctx, len(blobs), ba, len(commitments), ca, len(proofs), pa,
                                                                  C.byref(ok)))
        return bool(ok.value)

    # ---- batched additions ----------------------------------------------------------------
    def compute_cells_and_kzg_proofs_batch(self, blobs):
        """List of blobs -> (status list, cells[b][128], proofs[b][128]); host buffers."""
        n = len(blobs)
        if any(len(b) != BYTES_PER_BLOB for b in blobs):
            raise KzgError("InvalidLength")
        ba, _kb = _flat_ptrs(blobs, BYTES_PER_BLOB)
        cells, _ci, cpp = _out_ptrs(n, 128, BYTES_PER_CELL)
        proofs, _pi, ppp = _out_ptrs(n, 128, 48)
        st = (C.c_int32 * max(1, n))()
        self._check(self._lib.eth_kzg_amd_compute_cells_and_kzg_proofs_batch(self._ctx, n, _vp(ba), _vp(cpp), _vp(ppp), st))
        return list(st)[:n], _split(cells, n, 128, BYTES_PER_CELL), _split(proofs, n, 128, 48)

    def host_batch_buffers(self, n):
        """Caller-side buffers of the host-pointer batch ABI, allocated and touched once so that repeated calls measure
        the library and not the page faults of fresh output memory: (cells [n,128,2048] u8, proofs [n,128,48] u8,
        cell pointer tables, proof pointer tables)."""
        cells, ci, cpp = _out_ptrs(n, 128, BYTES_PER_CELL)
        proofs, pi, ppp = _out_ptrs(n, 128, 48)
        return {"cells": cells.reshape(n, 128, BYTES_PER_CELL), "proofs": proofs.reshape(n, 128, 48), "_ci": ci, "_pi": pi,
                "cpp": cpp, "ppp": ppp, "status": (C.c_int32 * max(1, n))()}

    def compute_cells_and_kzg_proofs_batch_np(self, blobs_np, bufs, want_proofs=True):
        """eth_kzg_amd_compute_cells_and_kzg_proofs_batch on a contiguous [n,131072] uint8 array (one pointer per blob, as
        a C caller would pass) into `bufs` from host_batch_buffers; returns the status list.  Only the C call happens here."""
        n = blobs_np.shape[0]
        assert blobs_np.dtype == np.uint8 and blobs_np.flags["C_CONTIGUOUS"] and blobs_np.size == n * BYTES_PER_BLOB
        ba = np.uint64(blobs_np.ctypes.data) + np.arange(max(1, n), dtype=np.uint64) * np.uint64(BYTES_PER_BLOB)
        self._check(self._lib.eth_kzg_amd_compute_cells_and_kzg_proofs_batch(
            self._ctx, n, _vp(ba), _vp(bufs["cpp"]), _vp(bufs["ppp"]) if want_proofs else None, bufs["status"]))
        return list(bufs["status"])[:n]

    def blob_to_kzg_commitment_batch(self, blobs):
        n = len(blobs)
        if any(len(b) != BYTES_PER_BLOB for b in blobs):
            raise KzgError("InvalidLength")
        ba, _kb = _ptr_array(blobs)
        outs = [C.create_string_buffer(48) for _ in range(n)]
        oa, _ko = _ptr_array(outs)
        st = (C.c_int32 * max(1, n))()
        self._check(self._lib.eth_kzg_amd_blob_to_kzg_commitment_batch(self._ctx, n, ba, oa, st))
        return list(st)[:n], [o.raw for o in outs]

    def recover_cells_and_kzg_proofs_batch(self, batch):
        """batch = [(cell_indices, cells), ...] -> (status list, cells[b][128], proofs[b][128])."""
        n = len(batch)
        keep = []
        lens = np.array([len(c) for _, c in batch] or [0], dtype=np.uint64)
        ilens = np.array([len(i) for i, _ in batch] or [0], dtype=np.uint64)
        cpp, ipp = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint64)
        for b, (idx, cells) in enumerate(batch):
            if any(len(c) != BYTES_PER_CELL for c in cells):
                raise KzgError("InvalidLength")
            ca, k1 = _flat_ptrs(cells, BYTES_PER_CELL)
            ia = np.array(idx, dtype=np.uint64) if len(idx) else np.zeros(1, np.uint64)
            keep += [ca, k1, ia]
            cpp[b], ipp[b] = ca.ctypes.data, ia.ctypes.data
        out_cells, _ci, ocp = _out_ptrs(n, 128, BYTES_PER_CELL)
        out_proofs, _pi, opp = _out_ptrs(n, 128, 48)
        st = (C.c_int32 * max(1, n))()
        self._check(self._lib.eth_kzg_amd_recover_cells_and_proofs_batch(
            self._ctx, n, _vp(lens), _vp(cpp), _vp(ilens), _vp(ipp), _vp(ocp), _vp(opp), st))
        return list(st)[:n], _split(out_cells, n, 128, BYTES_PER_CELL), _split(out_proofs, n, 128, 48)

    def compute_cells_and_kzg_proofs_device(self, n, d_blobs, d_cells, d_proofs, want_status=True, stream=None):
        """Device-resident flat buffers (integer device addresses, e.g. torch tensor .data_ptr())."""
        st = (C.c_int32 * max(1, n))() if want_status else None
        self._check(self._lib.eth_kzg_amd_compute_cells_and_kzg_proofs_device(
            self._ctx, n, C.c_void_p(d_blobs), C.c_void_p(d_cells) if d_cells else None,
            C.c_void_p(d_proofs) if d_proofs else None, st, C.c_void_p(stream) if stream else None))
        return list(st)[:n] if want_status else None

    def recover_cells_and_kzg_proofs_device(self, n, d_cells, present, d_out_cells, d_out_proofs, stream=None):
        """Device-resident recovery: d_cells = flat [n][128][2048] buffer in HBM (integer address), present[b] = iterable
        of the cell indices of blob b that hold data.  Returns the per-blob status list; outputs stay on the device."""
        masks = present_masks(n, present)
        st = (C.c_int32 * max(1, n))()
        self._check(self._lib.eth_kzg_amd_recover_cells_and_proofs_device(
            self._ctx, n, C.c_void_p(d_cells), _vp(masks), C.c_void_p(d_out_cells) if d_out_cells else None,
            C.c_void_p(d_out_proofs) if d_out_proofs else None, st, C.c_void_p(stream) if stream else None))
        return list(st)[:n]

    # ---- multi-GPU (include/c_eth_kzg.h): the library's own RCCL communicator and the single-process fan-out
    @staticmethod
    def comm_unique_id():
        """128 bytes from ncclGetUniqueId (rank 0 calls this and distributes them)."""
        out = C.create_string_buffer(128)
        res = load_library().eth_kzg_amd_comm_unique_id(out)
        if res.status != 0:
            msg = C.cast(res.error_msg, C.c_char_p).value.decode() if res.error_msg else "error"
            load_library().eth_kzg_free_error_message(res.error_msg)
            raise KzgError(msg)
        return out.raw

    def comm_probe(self):
        """Local and cheap: raises KzgError unless RCCL can be bound and this context has no communicator yet; returns the
        library file that was bound (and whether it was the copy the process had already mapped)."""
        buf = C.create_string_buffer(512)
        self._check(self._lib.eth_kzg_amd_comm_probe(self._ctx, buf, 512))
        return buf.value.decode()

    def comm_init(self, unique_id, rank, world):
        """COLLECTIVE (ncclCommInitRank): every rank enters or none -- agree on comm_probe() first."""
        self._check(self._lib.eth_kzg_amd_comm_init(self._ctx, unique_id, int(rank), int(world)))

    def comm_info(self):
        """(rank, world) as the library's communicator itself reports them."""
        r, w = C.c_int(-1), C.c_int(-1)
        self._check(self._lib.eth_kzg_amd_comm_info(self._ctx, C.byref(r), C.byref(w)))
        return r.value, w.value

    def all_gather(self, d_send, d_recv, bytes_per_rank, stream=None):
        """ncclAllGather of bytes_per_rank bytes from every rank's d_send into d_recv (device addresses), on `stream`
        (None: the context's stream, synchronised)."""
        self._check(self._lib.eth_kzg_amd_all_gather(self._ctx, C.c_void_p(d_send), C.c_void_p(d_recv), int(bytes_per_rank),
                                                     C.c_void_p(stream) if stream else None))

    def comm_destroy(self):
        self._lib.eth_kzg_amd_comm_destroy(self._ctx)

    @staticmethod
    def compute_cells_and_kzg_proofs_batch_multi(contexts, blobs_np, bufs):
        """eth_kzg_amd_compute_cells_and_kzg_proofs_batch_multi: one host-pointer batch cut into contiguous slices over
        `contexts` (one per GPU), buffers as in compute_cells_and_kzg_proofs_batch_np."""
        lib = load_library()
        n = blobs_np.shape[0]
        ba = np.uint64(blobs_np.ctypes.data) + np.arange(max(1, n), dtype=np.uint64) * np.uint64(BYTES_PER_BLOB)
        ctxs = (C.c_void_p * len(contexts))(*[c.handle for c in contexts])
        contexts[0]._check(lib.eth_kzg_amd_compute_cells_and_kzg_proofs_batch_multi(
            ctxs, len(contexts), n, _vp(ba), _vp(bufs["cpp"]), _vp(bufs["ppp"]), bufs["status"]))
        return list(bufs["status"])[:n]

    def verify_cell_kzg_proof_batch_device(self, n, d_commitments, d_cell_indices, d_cells, d_proofs, stream=None, leaf_transcript=False):
        """Device-resident verification: integer device addresses of n*48 commitment bytes (one per cell), n uint64 indices,
        n*2048 cell bytes, n*48 proof bytes.  leaf_transcript=True: eth_kzg_amd_verify_cell_kzg_proof_batch_device_ex with
        ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT -- cells and proofs are hashed where they lie and never copied to the host."""
        ok = C.c_bool(False)
        if leaf_transcript:
            self._check(self._lib.eth_kzg_amd_verify_cell_kzg_proof_batch_device_ex(
                self._ctx, int(n), C.c_void_p(d_commitments), C.c_void_p(d_cell_indices), C.c_void_p(d_cells), C.c_void_p(d_proofs),
                VERIFY_LEAF_TRANSCRIPT, C.byref(ok), C.c_void_p(stream) if stream else None))
            return bool(ok.value)
        self._check(self._lib.eth_kzg_amd_verify_cell_kzg_proof_batch_device(
            self._ctx, int(n), C.c_void_p(d_commitments), C.c_void_p(d_cell_indices), C.c_void_p(d_cells), C.c_void_p(d_proofs),
            C.byref(ok), C.c_void_p(stream) if stream else None))
        return bool(ok.value)

    def blob_to_kzg_commitment_device(self, n, d_blobs, d_out, want_status=True, stream=None):
        st = (C.c_int32 * max(1, n))() if want_status else None
        self._check(self._lib.eth_kzg_amd_blob_to_kzg_commitment_device(
            self._ctx, n, C.c_void_p(d_blobs), C.c_void_p(d_out), st, C.c_void_p(stream) if stream else None))
        return list(st)[:n] if want_status else None

    # ---- EIP-4844 proofs for many blobs (eth_kzg_amd_compute_*_kzg_proof_batch / _device) ----
    def compute_blob_kzg_proof_batch(self, blobs, commitments):
        """Lists of blobs and commitments -> (status list, proofs): compute_blob_kzg_proof for every pair in one call.  status[b]: 0 ok,
        1 the blob holds a non-canonical field element, 2 the commitment is not a valid point (the proof of such a blob is 48 zero bytes)."""
        n = len(blobs)
        if len(commitments) != n or any(len(b) != BYTES_PER_BLOB for b in blobs) or any(len(c) != 48 for c in commitments):
            raise KzgError("InvalidLength")
        ba, _kb = _flat_ptrs(blobs, BYTES_PER_BLOB)
        ca, _kc = _flat_ptrs(commitments, 48)
        out = np.zeros(max(1, n) * 48, dtype=np.uint8)
        oa = np.uint64(out.ctypes.data) + np.arange(max(1, n), dtype=np.uint64) * np.uint64(48)
        st = (C.c_int32 * max(1, n))()
        self._check(self._lib.eth_kzg_amd_compute_blob_kzg_proof_batch(self._ctx, n, _vp(ba), _vp(ca), _vp(oa), st))
        raw = out.tobytes()
        return list(st)[:n], [raw[48 * b:48 * b + 48] for b in range(n)]

    def compute_kzg_proof_batch(self, blobs, zs):
        """Lists of blobs and 32-byte evaluation points -> (status list, proofs, ys): compute_kzg_proof for every pair in one call.
        status[b]: 0 ok, 1 the blob or z holds a non-canonical field element (outputs of such a blob are zero bytes)."""
        n = len(blobs)
        if len(zs) != n or any(len(b) != BYTES_PER_BLOB for b in blobs) or any(len(z) != 32 for z in zs):
            raise KzgError("InvalidLength")
        ba, _kb = _flat_ptrs(blobs, BYTES_PER_BLOB)
        za, _kz = _flat_ptrs(zs, 32)
        proofs, ys = np.zeros(max(1, n) * 48, dtype=np.uint8), np.zeros(max(1, n) * 32, dtype=np.uint8)
        pa = np.uint64(proofs.ctypes.data) + np.arange(max(1, n), dtype=np.uint64) * np.uint64(48)
        ya = np.uint64(ys.ctypes.data) + np.arange(max(1, n), dtype=np.uint64) * np.uint64(32)
        st = (C.c_int32 * max(1, n))()
        self._check(self._lib.eth_kzg_amd_compute_kzg_proof_batch(self._ctx, n, _vp(ba), _vp(za), _vp(pa), _vp(ya), st))
        rp, ry = proofs.tobytes(), ys.tobytes()
        return list(st)[:n], [rp[48 * b:48 * b + 48] for b in range(n)], [ry[32 * b:32 * b + 32] for b in range(n)]

    def compute_blob_kzg_proof_device(self, n, d_blobs, d_commitments, d_out_proofs, want_status=True, stream=None):
        """Device-resident flat buffers (integer device addresses): n * 131072 blob bytes, n * 48 commitment bytes -> n * 48 proof
        bytes; the Fiat-Shamir challenges are hashed on the GPU.  Returns the status list (None with want_status=False: then, with
        a stream, the call does not synchronise)."""
        st = (C.c_int32 * max(1, n))() if want_status else None
        self._check(self._lib.eth_kzg_amd_compute_blob_kzg_proof_device(
            self._ctx, n, C.c_void_p(d_blobs), C.c_void_p(d_commitments), C.c_void_p(d_out_proofs), st, C.c_void_p(stream) if stream else None))
        return list(st)[:n] if want_status else None

    def compute_kzg_proof_device(self, n, d_blobs, d_zs, d_out_proofs, d_out_ys, want_status=True, stream=None):
        """Device-resident compute_kzg_proof: n * 32 big-endian z bytes in, n * 48 proof and n * 32 y bytes out."""
        st = (C.c_int32 * max(1, n))() if want_status else None
        self._check(self._lib.eth_kzg_amd_compute_kzg_proof_device(
            self._ctx, n, C.c_void_p(d_blobs), C.c_void_p(d_zs), C.c_void_p(d_out_proofs), C.c_void_p(d_out_ys), st,
            C.c_void_p(stream) if stream else None))
        return list(st)[:n] if want_status else None

    def verify_blob_kzg_proof_batch_device(self, n, d_blobs, d_commitments, d_proofs, stream=None):
        """verify_blob_kzg_proof_batch on flat arrays in HBM (integer device addresses); synchronous.  Raises KzgError for
        malformed input, as the host form."""
        ok = C.c_bool(False)
        self._check(self._lib.eth_kzg_amd_verify_blob_kzg_proof_batch_device(
            self._ctx, int(n), C.c_void_p(d_blobs), C.c_void_p(d_commitments), C.c_void_p(d_proofs), C.byref(ok),
            C.c_void_p(stream) if stream else None))
        return bool(ok.value)

    STAGES = ["blob_to_coeffs", "coeffs_to_cells", "fk20_scalars", "msm_fixed", "g1_ifft", "g1_fft", "compress", "g1_linmap"]

    def set_profiling(self, on):
        self._lib.eth_kzg_amd_set_profiling(self._ctx, int(bool(on)))

    def get_stage_times(self):
        """{stage: (milliseconds, kernel launches)} accumulated since the previous call."""
        n = len(self.STAGES)
        ms = (C.c_double * n)()
        ln = (C.c_uint64 * n)()
        self._lib.eth_kzg_amd_get_stage_times(self._ctx, ms, ln, n)
        return {s: (ms[i], int(ln[i])) for i, s in enumerate(self.STAGES)}

    def table_bytes(self):
        return int(self._lib.eth_kzg_amd_table_bytes(self._ctx))

    def window_bits(self):
        return int(self._lib.eth_kzg_amd_window_bits(self._ctx))

    def window_count(self):
        """Windows per 128-bit GLV half of the FK20 table in use (gathered additions per base = twice that)."""
        return int(self._lib.eth_kzg_amd_window_count(self._ctx))

    def linmap_info(self):
        """(constant multiplications, additions, doublings per blob, launches per call) of the compiled G1 linear map."""
        out = (C.c_int32 * 4)()
        self._lib.eth_kzg_amd_linmap_info(self._ctx, out)
        return tuple(out)
