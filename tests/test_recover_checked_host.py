"""A block's data columns recovered and checked against its commitments (eth_kzg_amd_recover_data_columns_checked / _device), on the CPU.

1. The two symbols are exported and mirrored in the Python package; the ABI version stays 6.
2. What they refuse before the context is touched -- exactly what eth_kzg_amd_recover_data_columns refuses.  A NULL context is passed, so
   reaching it would abort the process.  The empty call is Ok.
3. The Python wrappers check lengths before the call.
4. The host translation unit compiles on its own; a C99 consumer takes the address of both prototypes."""
import ctypes
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
kzg = importlib.import_module("rust-eth-kzg_amd")
SYMBOLS = ["eth_kzg_amd_recover_data_columns_checked", "eth_kzg_amd_recover_data_columns_checked_device"]


def _expect_invalid(lib, res):
    assert res.status == 1 and res.error_msg
    msg = ctypes.string_at(res.error_msg).decode()
    lib.eth_kzg_free_error_message(res.error_msg)
    assert msg.startswith("InvalidInput"), msg


def _calls(lib, n, cells=None, indices=None, n_columns=0, status=None, commitments=None, outputs=None):
    """the two calls on a NULL context with everything else as given (outputs: one pointer for all four)"""
    o = outputs
    return [lambda: lib.eth_kzg_amd_recover_data_columns_checked(None, n, commitments, n_columns, indices, cells, o, o, o, o, status),
            lambda: lib.eth_kzg_amd_recover_data_columns_checked_device(None, n, commitments, n_columns, indices, cells, o, o, o, o, status, None)]


def test_symbols_are_exported_and_mirrored_and_the_abi_version_stays():
    lib = kzg.load_library()
    assert lib.eth_kzg_amd_abi_version() == 6
    for name in SYMBOLS:
        assert name in kzg.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert hasattr(ctypes.CDLL(kzg.HOOKS_LIB_PATH), name), name
    for name in ("recover_data_columns_checked", "recover_data_columns_checked_device"):
        assert callable(getattr(kzg.DASContext, name)), name
    header = open(os.path.join(ROOT, "include", "c_eth_kzg.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header, name


def test_oversized_counts_are_rejected_before_the_context_is_looked_at():
    lib = kzg.load_library()
    something = ctypes.create_string_buffer(64)
    st = (ctypes.c_int32 * 4)()
    for n in (1 << 32, (1 << 24) + 1, (1 << 64) - 1):
        for call in _calls(lib, n) + _calls(lib, n, cells=something, indices=something, n_columns=64, status=st, commitments=something,
                                            outputs=something):
            _expect_invalid(lib, call())


def test_null_arrays_with_a_count_are_rejected_before_the_context_is_looked_at():
    lib = kzg.load_library()
    something = ctypes.create_string_buffer(64)
    st = (ctypes.c_int32 * 4)()
    for n in (1, 3, 1 << 24):
        for commitments in (None, something):  # the commitments are optional: they never change a refusal
            for kw in (dict(cells=None, indices=something, n_columns=64, status=st),          # no cells
                       dict(cells=something, indices=None, n_columns=64, status=st),          # no indices, with a count
                       dict(cells=something, indices=something, n_columns=64, status=None),   # no status
                       dict(cells=None, indices=None, n_columns=0, status=st)):
                for call in _calls(lib, n, commitments=commitments, outputs=something, **kw):
                    _expect_invalid(lib, call())


def test_an_empty_call_is_ok_and_touches_nothing():
    lib = kzg.load_library()
    for call in _calls(lib, 0) + _calls(lib, 0, n_columns=64):
        res = call()
        assert res.status == 0 and not res.error_msg


def test_python_wrappers_check_lengths_before_the_call():
    c = kzg.DASContext.__new__(kzg.DASContext)
    c._ctx = ctypes.c_void_p(None)
    cell, comm = bytes(kzg.BYTES_PER_CELL), bytes(48)
    for call in (lambda: c.recover_data_columns_checked([0, 1], [[cell]]),
                 lambda: c.recover_data_columns_checked([0, 1], [[cell], [cell, cell]]),
                 lambda: c.recover_data_columns_checked([0], [[cell[:-1]]]),
                 lambda: c.recover_data_columns_checked([0], [[cell]], [comm, comm]),     # two commitments for one blob
                 lambda: c.recover_data_columns_checked([0], [[cell]], [comm[:-1]]),      # 47 bytes
                 lambda: c.recover_data_columns_checked([0, 1], [[cell, cell], [cell, cell]], [comm])):
        with pytest.raises(kzg.KzgError, match="InvalidLength"):
            call()
    c._ctx = None  # (nothing for __del__ to free)


@pytest.mark.timeout(600)
def test_the_host_unit_compiles_and_both_prototypes_parse_in_c(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "-x", "hip", "--cuda-host-only", "-c", os.path.join(csrc, "data_columns.hip"),
                           "-o", str(tmp_path / "data_columns.host.o")])  # plain build, the host pass only
    src = tmp_path / "consumer.c"
    src.write_text('#include "c_eth_kzg.h"\n'
                   "CResult (*const checked)(const DASContext *, uint64_t, const uint8_t *const *, uint64_t, const uint64_t *,\n"
                   "                         const uint8_t *const *const *, uint8_t *const *, uint8_t *const *, uint8_t *const *const *,\n"
                   "                         uint8_t *const *const *, int32_t *) = eth_kzg_amd_recover_data_columns_checked;\n"
                   "CResult (*const checked_device)(const DASContext *, uint64_t, const uint8_t *, uint64_t, const uint64_t *, const uint8_t *,\n"
                   "                                uint8_t *, uint8_t *, uint8_t *, uint8_t *, int32_t *, void *) =\n"
                   "    eth_kzg_amd_recover_data_columns_checked_device;\n"
                   "int main(void) { return checked == 0 || checked_device == 0; }\n")
    cc = shutil.which("cc") or shutil.which("gcc")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
