"""Caller-supplied trusted setups, the part that needs no GPU: the new C symbols, the argument checks of
eth_kzg_amd_das_context_new_with_setup (which come before a GPU is looked for), the JSON parser of the Python mirror, the host-side
G2 subgroup test, and the pure-Python G2 helper the GPU tests build their insecure setup with."""
import ctypes as C
import importlib
import json
import os
import re
import shutil
import subprocess

import pytest

import setup_material as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
kzg = importlib.import_module("rust-eth-kzg_amd")

NEW_SYMBOLS = ["eth_kzg_amd_das_context_new_with_setup", "eth_kzg_amd_das_context_new_with_setup_file", "eth_kzg_amd_setup_digest"]


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "c_eth_kzg.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = C.CDLL(kzg.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in kzg.EXPORTED_SYMBOLS
    assert "ETH_KZG_AMD_SETUP_NO_SUBGROUP_CHECK" in header and "ETH_KZG_AMD_SETUP_CHECK_POWERS" in header
    assert kzg.load_library().eth_kzg_amd_abi_version() == 6  # additions only


def _expect_err(ptr, res):
    lib = kzg.load_library()
    assert not ptr and res.status == 1 and res.error_msg
    msg = C.cast(res.error_msg, C.c_char_p).value.decode()
    lib.eth_kzg_free_error_message(res.error_msg)
    assert msg.startswith("ContextCreation("), msg
    return msg


def test_counts_and_null_arrays_are_rejected_before_the_gpu_is_looked_for():
    """n_g1 = 4095, n_g2 = 64 and a NULL array are NULL + Err naming the expected counts -- on a machine without a GPU too, where
    "no device" would otherwise be the first thing to go wrong."""
    lib = kzg.load_library()
    g1, g2 = sm.mainnet_points()
    b1, b2 = C.create_string_buffer(g1, len(g1)), C.create_string_buffer(g2, len(g2))
    a1, a2 = C.addressof(b1), C.addressof(b2)
    for args in ((a1, 4095, a2, 65), (a1, 4096, a2, 64), (a1, 0, a2, 0), (a1, 1 << 40, a2, 65), (None, 4096, a2, 65), (a1, 4096, None, 65)):
        res = kzg.CResult()
        p = lib.eth_kzg_amd_das_context_new_with_setup(args[0], args[1], args[2], args[3], 0, False, None, 0, 3.0, C.byref(res))
        msg = _expect_err(p, res)
        assert "InvalidInput" in msg and "4096" in msg and "65" in msg, msg
        if args[0] and args[2]:
            assert str(args[1]) in msg and str(args[3]) in msg, msg
    res = kzg.CResult()
    msg = _expect_err(lib.eth_kzg_amd_das_context_new_with_setup(a1, 4096, a2, 65, 0x80, False, None, 0, 3.0, C.byref(res)), res)
    assert "flags" in msg
    # the flat-file form: header and length are checked the same way
    flat = sm.flat_file(g1, g2)
    for bad in (flat[:-1], b"KZGSRS02" + flat[8:], flat[:8], sm.flat_file(g1[:-48], g2)):
        fb = C.create_string_buffer(bad, len(bad))
        res = kzg.CResult()
        msg = _expect_err(lib.eth_kzg_amd_das_context_new_with_setup_file(C.addressof(fb), len(bad), 0, False, None, 0, 3.0, C.byref(res)), res)
        assert "InvalidInput" in msg, msg
    res = kzg.CResult()
    _expect_err(lib.eth_kzg_amd_das_context_new_with_setup_file(None, 0, 0, False, None, 0, 3.0, C.byref(res)), res)
    with pytest.raises(kzg.KzgError, match="4096"):
        kzg.DASContext.from_trusted_setup(g1[:-48], g2, use_precomp=False)


def test_bad_g2_points_are_rejected_on_the_host():
    """The G2 list is validated before any GPU work: an undecodable point and a curve point off the subgroup are named by index; with the
    subgroup check waived the latter gets as far as the GPU (on a machine without one, that is the error)."""
    g1, g2 = sm.mainnet_points()
    off = sm.g2_compress(sm.g2_off_subgroup_point())
    bad = g2[:96 * 37] + off + g2[96 * 38:]
    with pytest.raises(kzg.KzgError, match=r"InvalidSetup: g2_monomial\[37\] is not in the prime-order subgroup"):
        kzg.DASContext.from_trusted_setup(g1, bad, use_precomp=False, table_budget_gb=3)
    # [tau^21]_2 plus a point of order 13 (tests/small_order.py): on the curve, and psi(Q) == [x]Q has to tell it from the subgroup
    import small_order
    plus13 = sm.g2_compress(sm.g2_add(small_order.g2_decode(g2[96 * 21:96 * 22]), small_order.g2_small_order_points()[13]))
    with pytest.raises(kzg.KzgError, match=r"InvalidSetup: g2_monomial\[21\] is not in the prime-order subgroup"):
        kzg.DASContext.from_trusted_setup(g1, g2[:96 * 21] + plus13 + g2[96 * 22:], use_precomp=False, table_budget_gb=3)
    junk = g2[:96 * 5] + bytes([g2[96 * 5] & 0x7f]) + g2[96 * 5 + 1:]  # compression flag cleared
    with pytest.raises(kzg.KzgError, match=r"g2_monomial\[5\] is not the encoding of a curve point"):
        kzg.DASContext.from_trusted_setup(g1, junk, use_precomp=False, table_budget_gb=3)
    wrong_gen = g2[96:192] + g2[96:]
    with pytest.raises(kzg.KzgError, match=r"g2_monomial\[0\] is not the standard G2 generator"):
        kzg.DASContext.from_trusted_setup(g1, wrong_gen, check_powers=True, use_precomp=False, table_budget_gb=3)
    with pytest.raises(kzg.KzgError, match=r"g1_monomial\[0\] is not the standard G1 generator"):
        kzg.DASContext.from_trusted_setup(g1[48:96] + g1[48:], g2, check_powers=True, use_precomp=False, table_budget_gb=3)


def _mainnet_json(extra=None, prefix="0x"):
    g1, g2 = sm.mainnet_points()
    doc = {"g1_monomial": [prefix + g1[48 * i:48 * i + 48].hex() for i in range(sm.N_G1)],
           "g2_monomial": [prefix + g2[96 * i:96 * i + 96].hex() for i in range(sm.N_G2)]}
    doc.update(extra or {})
    return json.dumps(doc)


def test_json_parser_round_trips_the_mainnet_file_and_ignores_g1_lagrange():
    g1, g2 = sm.mainnet_points()
    p1, p2 = kzg.parse_trusted_setup_json(_mainnet_json())
    assert b"".join(p1) == g1 and b"".join(p2) == g2
    # g1_lagrange is not needed and not looked at (crates/trusted_setup/src/lib.rs:111): garbage in it changes nothing
    q1, q2 = kzg.parse_trusted_setup_json(_mainnet_json({"g1_lagrange": ["not even hex", 7]}))
    assert (q1, q2) == (p1, p2)


def test_json_parser_rejects_malformed_entries():
    with pytest.raises(kzg.KzgError, match="0x"):
        kzg.parse_trusted_setup_json(_mainnet_json(prefix=""))
    doc = json.loads(_mainnet_json())
    for mutate, pattern in ((lambda d: d.pop("g2_monomial"), "g2_monomial is missing"),
                            (lambda d: d["g1_monomial"].__setitem__(3, "0x1234"), r"g1_monomial\[3\] has 2 bytes"),
                            (lambda d: d["g2_monomial"].__setitem__(1, "0xzz"), r"g2_monomial\[1\] is not hex")):
        d = json.loads(json.dumps(doc))
        mutate(d)
        with pytest.raises(kzg.KzgError, match=pattern):
            kzg.parse_trusted_setup_json(json.dumps(d))
    with pytest.raises(kzg.KzgError, match="not JSON"):
        kzg.parse_trusted_setup_json("{")


def test_python_g2_helper_matches_the_mainnet_file():
    """The helper's compression of the standard generator is g2_monomial[0]; its group law is a group law (on the curve, r kills the
    generator, (a + b) G = a G + b G); the constructed off-subgroup point is on the curve and survives r."""
    _, g2 = sm.mainnet_points()
    assert sm.g2_on_curve(sm.G2_GEN)
    assert sm.g2_compress(sm.G2_GEN) == g2[:96]
    assert sm.g2_mul(sm.G2_GEN, sm.R) is None
    a, b = 0x1234567, 0xfedcba9876543
    assert sm.g2_add(sm.g2_mul(sm.G2_GEN, a), sm.g2_mul(sm.G2_GEN, b)) == sm.g2_mul(sm.G2_GEN, a + b)
    assert sm.g2_compress(None) == bytes([0xc0]) + bytes(95)
    off = sm.g2_off_subgroup_point()
    assert sm.g2_on_curve(off) and sm.g2_mul(off, sm.R) is not None


@pytest.mark.timeout(600)
def test_host_g2_subgroup_test_against_the_definition(tmp_path):
    """csrc/host_pairing.cpp: the psi-endomorphism test against [r]Q = O -- multiples of the generator pass, curve points off the
    subgroup (its own and the one the Python helper constructs) fail, infinity passes as in the reference's checked parser."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "test_g2_subgroup")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_g2_subgroup.cpp"), "-o", exe])
    off = tmp_path / "off_subgroup.bin"
    import small_order
    planned = small_order.g2_encodings()  # points of order 13, 23, 2713 and [k][1]_2 + each of them
    assert len(planned) == 96 * small_order.N_G2_POINTS
    off.write_bytes(sm.g2_compress(sm.g2_off_subgroup_point()) + planned)
    out = subprocess.run([exe, sm.MAINNET_BIN, str(off)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "%d off it, 0 mismatches" % (7 + small_order.N_G2_POINTS) in out.stdout, out.stdout
    # the single-point use stays valid
    off.write_bytes(sm.g2_compress(sm.g2_off_subgroup_point()))
    out = subprocess.run([exe, sm.MAINNET_BIN, str(off)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "7 off it, 0 mismatches" in out.stdout, out.stdout + out.stderr
    off.write_bytes(planned[:95])  # and a file that is no multiple of 96 bytes is an error, not an empty list
    out = subprocess.run([exe, sm.MAINNET_BIN, str(off)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 1 and "cannot read" in out.stdout, out.stdout + out.stderr
