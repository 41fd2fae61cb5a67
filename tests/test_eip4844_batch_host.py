"""CPU-side checks of the batched / device-resident EIP-4844 proof entry points (include/c_eth_kzg.h:
eth_kzg_amd_compute_blob_kzg_proof_batch / _device, eth_kzg_amd_compute_kzg_proof_batch / _device,
eth_kzg_amd_verify_blob_kzg_proof_batch_device).  No compute call is made here: the count check comes before the context is looked
at, so a NULL context is never reached.  The symbol lists themselves (header / Python / .so / .a, the hook absent from the product
library) are tests/test_abi_exports.py's business."""
import ctypes
import importlib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
kzg = importlib.import_module("rust-eth-kzg_amd")
if not os.path.exists(kzg.LIB_PATH):  # fresh checkout: cross-compile the HIP extension (no GPU needed, a few minutes)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rust-eth-kzg_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1))])

NEW_SYMBOLS = [
    "eth_kzg_amd_compute_blob_kzg_proof_batch", "eth_kzg_amd_compute_kzg_proof_batch",
    "eth_kzg_amd_compute_blob_kzg_proof_device", "eth_kzg_amd_compute_kzg_proof_device",
    "eth_kzg_amd_verify_blob_kzg_proof_batch_device",
]


def test_oversized_counts_are_rejected_before_the_context_is_looked_at():
    lib = kzg.load_library()
    n = 1 << 32

    def expect_invalid(res):
        assert res.status == 1 and res.error_msg
        msg = ctypes.string_at(res.error_msg).decode()
        lib.eth_kzg_free_error_message(res.error_msg)
        assert msg.startswith("InvalidInput"), msg

    expect_invalid(lib.eth_kzg_amd_compute_blob_kzg_proof_batch(None, n, None, None, None, None))
    expect_invalid(lib.eth_kzg_amd_compute_kzg_proof_batch(None, n, None, None, None, None, None))
    expect_invalid(lib.eth_kzg_amd_compute_blob_kzg_proof_device(None, n, None, None, None, None, None))
    expect_invalid(lib.eth_kzg_amd_compute_kzg_proof_device(None, n, None, None, None, None, None, None))
    ok = ctypes.c_bool(True)
    expect_invalid(lib.eth_kzg_amd_verify_blob_kzg_proof_batch_device(None, n, None, None, None, ctypes.byref(ok), None))
    expect_invalid(lib.eth_kzg_amd_compute_blob_kzg_proof_batch(None, (1 << 24) + 1, None, None, None, None))  # the bound itself


def test_additions_keep_the_abi_version():
    lib = kzg.load_library()
    assert lib.eth_kzg_amd_abi_version() == 6
    for name in NEW_SYMBOLS:
        assert name in kzg.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "eth_kzg_amd_test_sha256_many" in kzg.TEST_HOOK_SYMBOLS and "eth_kzg_amd_test_sha256_many" not in kzg.EXPORTED_SYMBOLS


def test_python_methods_exist_and_check_lengths_before_the_call():
    for name in ("compute_blob_kzg_proof_batch", "compute_kzg_proof_batch", "compute_blob_kzg_proof_device", "compute_kzg_proof_device",
                 "verify_blob_kzg_proof_batch_device"):
        assert callable(getattr(kzg.DASContext, name)), name
    # a wrong byte length cannot cross the C ABI: the wrappers raise before the FFI call (no context needed to get that far)
    c = kzg.DASContext.__new__(kzg.DASContext)
    c._ctx = ctypes.c_void_p(None)
    blob = bytes(kzg.BYTES_PER_BLOB)
    for call in (lambda: c.compute_blob_kzg_proof_batch([blob], [bytes(47)]), lambda: c.compute_blob_kzg_proof_batch([blob[:-1]], [bytes(48)]),
                 lambda: c.compute_blob_kzg_proof_batch([blob], []), lambda: c.compute_kzg_proof_batch([blob], [bytes(33)]),
                 lambda: c.compute_kzg_proof_batch([blob, blob], [bytes(32)])):
        try:
            call()
            raise AssertionError("no InvalidLength")
        except kzg.KzgError as e:
            assert "InvalidLength" in str(e)
