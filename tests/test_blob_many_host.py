"""eth_kzg_amd_verify_blob_kzg_proof_many / _many_device, on the CPU.

1. The host statement in csrc/verify_host.hpp -- blob_item_status / blob_item_live / blob_item_verified over all 2 x 3 x 2 x 2
   combinations of (blob bad, what the decoding left for the commitment: 0 / 1 / 2, proof bad, the pair passed), the challenge z as the
   leaf takes it, the passes at the blob source's pass size -- through a stand-alone program (tests/c/test_blob_many.cpp, its own main)
   built with hipcc's host pass, once plain and once with AddressSanitizer + UBSan and run directly, against values written here from
   hashlib and Python integers (tests/blob_many.py).  Nothing is loaded into Python under a sanitizer.
2. The statement in Python on itself: a refused blob's y is zero bytes, z is hashed from the bytes as they stand, the closed forms the
   GPU tests rely on (a monomial blob evaluates to z^j, a point of the domain to the element at its place).
3. The drop-in boundary: the two symbols are exported, the hooks by the hooks library only, the ABI version stays 6, and the call-level
   InvalidInput cases come before the context is touched (a NULL context is never reached), through the product library."""
import ctypes
import importlib
import itertools
import os
import shutil
import subprocess

import pytest

import blob_many as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
kzg = importlib.import_module("rust-eth-kzg_amd")
R = BM.R


# ---- 1. csrc/verify_host.hpp through a stand-alone program ------------------------------------------------------------------------------------
def _cases():
    lines, want = [], []
    for blob_bad, cst, pbad, passed in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1)):
        pst = 2 * pbad
        lines.append("merge %d %d %d %d" % (blob_bad, cst, pst, passed))
        st, live, ver = BM.merge(blob_bad, cst, pst, passed)
        want.append("merge %d %d %d" % (st, live, ver))
    for tag, commitment in ((b"blobmany", BM.INF), (b"blobman2", b"\xff" * 48), (b"blobmany", bytes(48))):
        lines.append("challenge %s %s" % (tag.hex(), commitment.hex()))
        want.append("challenge " + BM.fr_be(BM.blob_challenge(BM.seeded_cheap_blob(tag), commitment)).hex())
    for n in (0, 1, BM.PASS - 1, BM.PASS, BM.PASS + 1, 300, 3 * BM.PASS):
        lines.append("bounds %d" % n)
        want.append("bounds " + ",".join(str(v) for v in BM.PM.pass_bounds(n, BM.PASS)))
    lines.append("limits")
    want.append("limits %d %d" % (BM.MAX_ITEMS, BM.PASS))
    return lines, want


@pytest.fixture(scope="module", params=list(BUILDS))
def printed(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("blob_many_" + request.param)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, cases = str(tmp / "test_blob_many"), str(tmp / "cases.txt")
    subprocess.check_call([hipcc, *BUILDS[request.param], "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_blob_many.cpp"), "-o", exe])
    lines, want = _cases()
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    return lines, want, got


@pytest.mark.timeout(600)
@pytest.mark.parametrize("what,count", [("merge", 24), ("challenge", 3), ("bounds", 7), ("limits", 1)])
def test_host_statement(printed, what, count):
    lines, want, got = printed
    rows = [(l, g, w) for l, g, w in zip(lines, got, want) if l.split()[0] == what]
    assert len(rows) == count
    for l, g, w in rows:
        assert g == w, (l[:80], g[:120], w[:120])


def test_the_merge_follows_the_order_of_the_issue():
    """written out once more, from the sentences of the issue and not from the case analysis in blob_many.merge"""
    for blob_bad, cst, pbad, passed in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1)):
        st, live, ver = BM.merge(blob_bad, cst, 2 * pbad, passed)
        if blob_bad:
            assert st == 1  # also when a point is bad as well
        elif cst or pbad:
            assert st == 2
        else:
            assert st == 0 and ver == bool(passed)
        assert live == (st == 0)
        if st != 0:
            assert ver is False


# ---- 2. the statement on itself ---------------------------------------------------------------------------------------------------------------
def test_statement_of_the_point_item():
    blob = BM.seeded_cheap_blob(b"blobmany")
    bad = BM.with_element(blob, 1023, R)
    assert not BM.blob_is_bad(blob) and BM.blob_is_bad(bad) and BM.blob_is_bad(BM.with_element(blob, 4095, (1 << 256) - 1))
    c, z, y, p = BM.point_item((bad, BM.INF, BM.INF))
    assert y == bytes(32) and (c, p) == (BM.INF, BM.INF)
    assert int.from_bytes(z, "big") == BM.blob_challenge(bad, BM.INF) != BM.blob_challenge(blob, BM.INF)  # hashed as the bytes stand
    assert BM.point_item((blob, BM.INF, BM.INF))[1] != BM.point_item((blob, b"\xff" * 48, BM.INF))[1]  # the commitment's bytes too


def test_closed_forms_of_the_evaluation():
    z = int.from_bytes(b"blob-many:z".ljust(31, b"\0"), "big") % R
    for j in (0, 1, 32, 1024, 4095):
        assert BM.blob_eval(BM.monomial_blob(j), z) == pow(z, j, R), j
    blob = BM.seeded_cheap_blob(b"blobmany")
    for k in (1, 2048, 4095):  # omega^k is the point of element brp(k)
        at = BM.brp(k, 12)
        assert BM.blob_eval(blob, pow(BM.W4096, k, R)) == int.from_bytes(blob[32 * at:32 * at + 32], "big"), k
    assert BM.blob_eval(BM.blob_of([5] * BM.N), z) == 5 and BM.blob_eval(bytes(BM.BLOB_BYTES), z) == 0


# ---- 3. the drop-in boundary ---------------------------------------------------------------------------------------------------------------
NEW = ["eth_kzg_amd_verify_blob_kzg_proof_many", "eth_kzg_amd_verify_blob_kzg_proof_many_device"]
HOOKS = ["eth_kzg_amd_test_blob_eval_at", "eth_kzg_amd_test_verify_blob_kzg_proof_many_sums"]


def test_symbols_are_listed_and_exported_and_the_hooks_are_in_the_hooks_library_only():
    assert set(NEW) <= set(kzg.EXPORTED_SYMBOLS) and not set(HOOKS) & set(kzg.EXPORTED_SYMBOLS)
    assert set(HOOKS) <= set(kzg.TEST_HOOK_SYMBOLS) and not set(NEW) & set(kzg.TEST_HOOK_SYMBOLS)
    product, hooks = ctypes.CDLL(kzg.LIB_PATH), ctypes.CDLL(kzg.HOOKS_LIB_PATH)
    for name in NEW:
        assert hasattr(product, name) and hasattr(hooks, name), name
    for name in HOOKS:
        assert hasattr(hooks, name) and not hasattr(product, name), name
    assert product.eth_kzg_amd_abi_version() == 6 and hooks.eth_kzg_amd_abi_version() == 6
    assert callable(kzg.DASContext.verify_blob_kzg_proof_many) and callable(kzg.DASContext.verify_blob_kzg_proof_many_device)


def test_counts_and_null_arrays_are_refused_before_the_context_is_touched():
    product = ctypes.CDLL(kzg.LIB_PATH)  # the product library itself, whatever the tests load otherwise
    P, U64 = ctypes.c_void_p, ctypes.c_uint64
    host, dev = product.eth_kzg_amd_verify_blob_kzg_proof_many, product.eth_kzg_amd_verify_blob_kzg_proof_many_device
    host.restype = dev.restype = kzg.CResult
    host.argtypes = [P, U64, P, P, P, P, P]
    dev.argtypes = [P, U64, P, P, P, P, P, P]
    product.eth_kzg_free_error_message.argtypes = [P]

    def expect_invalid(res):
        assert res.status == 1 and res.error_msg
        msg = ctypes.string_at(res.error_msg).decode()
        product.eth_kzg_free_error_message(res.error_msg)
        assert msg.startswith("InvalidInput"), msg

    one = (ctypes.c_void_p * 1)(ctypes.addressof(ctypes.create_string_buffer(48)))
    ver, st = (ctypes.c_bool * 1)(), (ctypes.c_int32 * 1)()
    for big in (1 << 32, (1 << 24) + 1):
        expect_invalid(host(None, big, one, one, one, ver, st))
        expect_invalid(dev(None, big, one, one, one, ver, st, None))
    for hole in range(3):  # a NULL array with n = 1 and a NULL context
        args = [one, one, one]
        args[hole] = None
        expect_invalid(host(None, 1, *args, ver, st))
        expect_invalid(dev(None, 1, *args, ver, st, None))
    expect_invalid(host(None, 1, one, one, one, None, st))
    expect_invalid(dev(None, 1, one, one, one, None, st, None))
