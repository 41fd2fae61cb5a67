"""eth_kzg_amd_blobs_to_data_columns / _device, on the CPU: the drop-in boundary.

The two symbols are declared in include/c_eth_kzg.h, exported by the product and the hooks library and mirrored in Python; the kernel's
hook is in the hooks library only; the ABI version stays 6.  Every call-level error of the contract is Err("InvalidInput...") BEFORE the
context is touched -- the calls are made with a NULL context through the product library, which aborts the process if it is ever looked
at -- and an empty call is Ok."""
import ctypes
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
kzg = importlib.import_module("rust-eth-kzg_amd")
NEW = ["eth_kzg_amd_blobs_to_data_columns", "eth_kzg_amd_blobs_to_data_columns_device"]
HOOK = "eth_kzg_amd_test_blob_to_columns"
VERIFY = 1  # ETH_KZG_AMD_COLUMNS_VERIFY_PROOFS


def _header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_are_declared_exported_and_mirrored():
    text, code = _header("c_eth_kzg.h")
    assert re.search(r"#define\s+ETH_KZG_AMD_COLUMNS_VERIFY_PROOFS\s+1u", code) and kzg.COLUMNS_VERIFY_PROOFS == VERIFY
    for name in NEW:
        assert re.search(r"\bCResult\s+%s\s*\(" % name, code), name
        assert name in kzg.EXPORTED_SYMBOLS and name not in kzg.TEST_HOOK_SYMBOLS
    assert re.search(r"\bint\s+%s\s*\(" % HOOK, _header("c_eth_kzg_test_hooks.h")[1]) and HOOK not in code
    assert HOOK in kzg.TEST_HOOK_SYMBOLS and HOOK not in kzg.EXPORTED_SYMBOLS
    product, hooks = ctypes.CDLL(kzg.LIB_PATH), ctypes.CDLL(kzg.HOOKS_LIB_PATH)
    for name in NEW:
        assert hasattr(product, name) and hasattr(hooks, name), name
    assert hasattr(hooks, HOOK) and not hasattr(product, HOOK)
    assert product.eth_kzg_amd_abi_version() == 6 and hooks.eth_kzg_amd_abi_version() == 6
    assert callable(kzg.DASContext.blobs_to_data_columns) and callable(kzg.DASContext.blobs_to_data_columns_device)
    assert callable(kzg.DASContext.test_blob_to_columns)


@pytest.fixture(scope="module")
def calls():
    product = ctypes.CDLL(kzg.LIB_PATH)  # the product library itself, whatever the tests load otherwise
    P, U64, U32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    host, dev = product.eth_kzg_amd_blobs_to_data_columns, product.eth_kzg_amd_blobs_to_data_columns_device
    host.restype = dev.restype = kzg.CResult
    host.argtypes = [P, U64, P, P, P, U32, P, P, P, P]
    dev.argtypes = [P, U64, P, P, P, U32, P, P, P, P, P]
    product.eth_kzg_free_error_message.argtypes = [P]

    def run(n, blobs, commitments, proofs, flags, out_cells, out_proofs, verified, status):
        """both forms with a NULL context -> their two results (status, message)"""
        out = []
        for res in (host(None, n, blobs, commitments, proofs, flags, out_cells, out_proofs, verified, status),
                    dev(None, n, blobs, commitments, proofs, flags, out_cells, out_proofs, verified, status, None)):
            msg = ctypes.string_at(res.error_msg).decode() if res.error_msg else None
            if res.error_msg:
                product.eth_kzg_free_error_message(res.error_msg)
            out.append((res.status, msg))
        return out
    return run


def _invalid(results):
    for status, msg in results:
        assert status == 1 and msg and msg.startswith("InvalidInput"), (status, msg)


def test_call_level_errors_come_before_the_context(calls):
    some = (ctypes.c_void_p * 1)(ctypes.addressof(ctypes.create_string_buffer(48)))  # a non-NULL array; never dereferenced
    ver, st = (ctypes.c_bool * 1)(), (ctypes.c_int32 * 1)()
    for flags in (2, 3, 4, 1 << 31, 0xFFFFFFFE):  # any other flag bit, with and without the known one, also in an empty call
        _invalid(calls(1, some, some, some, flags, some, some, ver, st))
        _invalid(calls(0, None, None, None, flags, None, None, None, None))
    for n in ((1 << 24) + 1, 1 << 32, (1 << 64) - 1):
        for flags in (0, VERIFY):
            _invalid(calls(n, some, some, some, flags, some, some, ver, st))
    for flags in (0, VERIFY):  # blobs NULL with n_blobs > 0
        _invalid(calls(1, None, some, some, flags, some, some, ver, st))
    _invalid(calls(1, some, some, None, VERIFY, some, None, ver, st))  # proofs NULL under the flag, out_proofs not asked for
    _invalid(calls(1, some, some, None, VERIFY, None, None, ver, st))
    _invalid(calls(1, some, None, None, 0, some, some, None, st))      # proofs NULL with out_proofs given
    _invalid(calls(1, some, None, some, VERIFY, some, some, ver, st))  # commitments NULL under the flag
    _invalid(calls(1, some, some, some, VERIFY, some, some, None, st))  # verified NULL under the flag


def test_an_empty_call_is_ok_and_touches_nothing(calls):
    for flags in (0, VERIFY):
        assert calls(0, None, None, None, flags, None, None, None, None) == [(0, None)] * 2
    some = (ctypes.c_void_p * 1)(ctypes.addressof(ctypes.create_string_buffer(48)))
    ver, st = (ctypes.c_bool * 1)(True), (ctypes.c_int32 * 1)(7)
    assert calls(0, some, some, some, VERIFY, some, some, ver, st) == [(0, None)] * 2
    assert ver[0] is True and st[0] == 7


def test_the_python_mirror_refuses_wrong_lengths_before_the_call():
    blob, p = bytes(131072), bytes([0xC0]) + bytes(47)
    for item in ((blob[:-1], p, [p] * 128), (blob, p[:-1], [p] * 128), (blob, None, [p] * 127), (blob, None, [p] * 127 + [p[:-1]])):
        with pytest.raises(kzg.KzgError, match="InvalidLength"):
            kzg.DASContext.blobs_to_data_columns(None, [item], verify=item[1] is not None)
