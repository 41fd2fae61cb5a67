"""eth_kzg_amd_verify_kzg_proof_many / _many_device, on the CPU.

1. The statement (tests/point_many.py) on itself: the passes of a call, what the weights hang on, the pair of a range against the
   per-item pairs, and the algebra of the degenerate items.
2. The host statement in csrc/verify_host.hpp -- PointProofTranscript::leaf / seed, the weights under that seed, point_pass_end,
   point_item_status -- through a stand-alone program (tests/c/test_point_many.cpp, its own main) built with hipcc's host pass, once plain
   and once with AddressSanitizer + UBSan and run directly, against values written here from hashlib and Python integers.  Nothing is
   loaded into Python under a sanitizer.
3. The drop-in boundary: the two symbols are exported, the hook by the hooks library only, the ABI version stays 6, and the call-level
   InvalidInput cases come before the context is touched (a NULL context is never reached)."""
import ctypes
import importlib
import os
import random
import shutil
import subprocess

import pytest

import oracle_lib
import point_many as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
kzg = importlib.import_module("rust-eth-kzg_amd")
R = PM.R


def _rb(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


# ---- 1. the statement ----------------------------------------------------------------------------------------------------------------------
def test_pass_bounds():
    assert PM.pass_bounds(0) == [0]
    assert PM.pass_bounds(1) == [0, 1]
    assert PM.pass_bounds(PM.PASS) == [0, PM.PASS]
    assert PM.pass_bounds(PM.PASS + 1) == [0, PM.PASS, PM.PASS + 1]
    assert PM.pass_bounds(200, 96) == [0, 96, 192, 200]


def test_one_byte_of_one_item_moves_every_weight_and_positions_restart_per_pass():
    rng = random.Random("point-many-host:weights")
    items = [(_rb(rng, 48), _rb(rng, 32), _rb(rng, 32), _rb(rng, 48)) for _ in range(9)]
    bounds, passes = PM.call_statement(items, [2] * 9, pass_size=5)
    assert bounds == [0, 5, 9] and [len(p.rho) for p in passes] == [5, 4]
    assert all(0 < r < (1 << 127) for p in passes for r in p.rho)
    assert passes[1].rho[0] == PM.weight(passes[1].seed, 0) != passes[0].rho[0]  # position in the PASS, under the pass's own seed
    for field in range(4):
        changed = list(items)
        it = list(items[7])
        it[field] = it[field][:-1] + bytes([it[field][-1] ^ 1])
        changed[7] = tuple(it)
        _, passes2 = PM.call_statement(changed, [2] * 9, pass_size=5)
        assert passes2[0].rho == passes[0].rho and passes2[0].seed == passes[0].seed
        assert all(a != b for a, b in zip(passes[1].rho, passes2[1].rho)), field
    # the seed binds the number of items: a pass is not a prefix of a longer one
    assert PM.seed(passes[0].leaves[:4]) != PM.seed(passes[0].leaves)
    # an item refused at validation takes no part in any sum
    assert passes[0].pair(0, 5) == PM.INF + PM.INF


def test_the_pair_of_a_range_is_the_sum_of_its_items_pairs_and_degenerate_items_degenerate():
    deg = PM.degenerate_items()
    names = list(deg)
    items = [deg[k] for k in names] + [deg["constant-polynomial"]] * 2
    statuses = [PM.item_status(it) for it in items]
    assert statuses == [0] * len(items)
    st = PM.PassStatement(items, statuses)
    G = PM.generator()
    for i, it in enumerate(items):
        c, z, y, p = it
        rho, zi, yi = st.rho[i], int.from_bytes(z, "big"), int.from_bytes(y, "big")
        first = PM.g1_mul_int(p, rho)
        inner = oracle_lib.g1_msm(c + p + G, PM.fr_be(1) + PM.fr_be(zi) + PM.fr_be(-yi))  # C + z pi - y G
        assert st.pair(i, i + 1) == first + PM.g1_mul_int(inner, rho), i
    whole = st.pair(0, len(items))
    firsts = [st.pair(i, i + 1)[:48] for i in range(len(items))]
    seconds = [st.pair(i, i + 1)[48:] for i in range(len(items))]
    one = PM.fr_be(1) * len(items)
    assert whole == oracle_lib.g1_msm(b"".join(firsts), one) + oracle_lib.g1_msm(b"".join(seconds), one)
    at = {k: i for i, k in enumerate(names)}
    assert st.pair(at["zero-polynomial"], at["zero-polynomial"] + 1) == PM.INF + PM.INF
    assert st.pair(at["constant-polynomial"], at["constant-polynomial"] + 1) == PM.INF + PM.INF
    for k in ("cancels", "doubling", "equals-yG"):
        assert st.pair(at[k], at[k] + 1)[:48] != PM.INF, k                        # pi = G: the first sum is rho G
    assert st.pair(at["equals-yG"], at["equals-yG"] + 1)[48:] == PM.INF           # C + z pi - y G is the identity, pi is not: invalid
    assert st.pair(at["cancels"], at["cancels"] + 1)[48:] == PM.INF               # C + z pi is the identity and y = 0
    assert st.pair(at["doubling"], at["doubling"] + 1)[48:] == PM.g1_mul_int(G, 10 * st.rho[at["doubling"]])


def test_status_order_of_the_statement():
    good = PM.degenerate_items()["constant-polynomial"]
    for name, (item, status) in PM.error_order_items(good).items():
        assert PM.item_status(item) == status, name


# ---- 2. csrc/verify_host.hpp through a stand-alone program ------------------------------------------------------------------------------------
def _cases():
    """-> (lines of the case file, what each must print): a plain function of the seed"""
    rng = random.Random("point-many-host:1")
    lines, want = [], []
    items = [(_rb(rng, 48), _rb(rng, 32), _rb(rng, 32), _rb(rng, 48)) for _ in range(5)] + [(bytes(48), bytes(32), bytes(32), b"\xff" * 48)]
    for it in items:
        lines.append("leaf " + " ".join(f.hex() for f in it))
        want.append("leaf " + PM.leaf(it).hex())
    for n in (0, 1, 2, 5, 64, 65):
        leaves = [_rb(rng, 32) for _ in range(n)]
        lines.append("seed %d %s" % (n, b"".join(leaves).hex() or "-"))
        want.append("seed " + PM.seed(leaves).hex())
    for n in (1, 3, 130):
        s = _rb(rng, 32)
        lines.append("weights %s %d" % (s.hex(), n))
        want.append("weights " + ",".join("%032x" % PM.weight(s, i) for i in range(n)))
    for n, p in ((0, 16384), (1, 16384), (16384, 16384), (16385, 16384), (200, 96), (192, 96), (3, 1), ((1 << 24), 16384)):
        lines.append("bounds %d %d" % (n, p))
        want.append("bounds " + ",".join(str(v) for v in PM.pass_bounds(n, p)))
    rm1, r, top = (R - 1).to_bytes(32, "big"), R.to_bytes(32, "big"), b"\xff" * 32
    for cbad, pbad, z, y, status in ((0, 0, rm1, rm1, 0), (0, 0, bytes(32), bytes(32), 0), (0, 0, r, rm1, 1), (0, 0, rm1, r, 1), (0, 0, top, top, 1),
                                     (1, 0, r, rm1, 2), (0, 1, rm1, top, 2), (1, 1, bytes(32), bytes(32), 2), (0, 0, (R + 1).to_bytes(32, "big"), bytes(32), 1)):
        lines.append("status %d %d %s %s" % (cbad, pbad, z.hex(), y.hex()))
        want.append("status %d" % status)
    return lines, want


@pytest.fixture(scope="module", params=list(BUILDS))
def printed(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("point_many_" + request.param)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, cases = str(tmp / "test_point_many"), str(tmp / "cases.txt")
    subprocess.check_call([hipcc, *BUILDS[request.param], "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_point_many.cpp"), "-o", exe])
    lines, want = _cases()
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    return lines, want, got


@pytest.mark.timeout(600)
@pytest.mark.parametrize("what,count", [("leaf", 6), ("seed", 6), ("weights", 3), ("bounds", 8), ("status", 9)])
def test_host_statement_equals_hashlib(printed, what, count):
    lines, want, got = printed
    rows = [(l, g, w) for l, g, w in zip(lines, got, want) if l.split()[0] == what]
    assert len(rows) == count
    for l, g, w in rows:
        assert g == w, (l[:80], g[:120], w[:120])


# ---- 3. the drop-in boundary ---------------------------------------------------------------------------------------------------------------
NEW = ["eth_kzg_amd_verify_kzg_proof_many", "eth_kzg_amd_verify_kzg_proof_many_device"]
HOOK = "eth_kzg_amd_test_verify_kzg_proof_many_sums"


def test_symbols_are_listed_and_exported_and_the_hook_is_in_the_hooks_library_only():
    assert set(NEW) <= set(kzg.EXPORTED_SYMBOLS) and HOOK not in kzg.EXPORTED_SYMBOLS
    assert HOOK in kzg.TEST_HOOK_SYMBOLS and not set(NEW) & set(kzg.TEST_HOOK_SYMBOLS)
    product, hooks = ctypes.CDLL(kzg.LIB_PATH), ctypes.CDLL(kzg.HOOKS_LIB_PATH)
    for name in NEW:
        assert hasattr(product, name) and hasattr(hooks, name), name
    assert hasattr(hooks, HOOK) and not hasattr(product, HOOK)
    assert product.eth_kzg_amd_abi_version() == 6 and hooks.eth_kzg_amd_abi_version() == 6
    assert callable(kzg.DASContext.verify_kzg_proof_many) and callable(kzg.DASContext.verify_kzg_proof_many_device)


def test_counts_and_null_arrays_are_refused_before_the_context_is_touched():
    lib = kzg.load_library()

    def expect_invalid(res):
        assert res.status == 1 and res.error_msg
        msg = ctypes.string_at(res.error_msg).decode()
        lib.eth_kzg_free_error_message(res.error_msg)
        assert msg.startswith("InvalidInput"), msg

    one = (ctypes.c_void_p * 1)(ctypes.addressof(ctypes.create_string_buffer(48)))
    ver, st = (ctypes.c_bool * 1)(), (ctypes.c_int32 * 1)()
    big = (1 << 24) + 1
    expect_invalid(lib.eth_kzg_amd_verify_kzg_proof_many(None, big, one, one, one, one, ver, st))
    expect_invalid(lib.eth_kzg_amd_verify_kzg_proof_many_device(None, big, one, one, one, one, ver, st, None))
    for hole in range(4):  # a NULL array with n = 1
        args = [one, one, one, one]
        args[hole] = None
        expect_invalid(lib.eth_kzg_amd_verify_kzg_proof_many(None, 1, *args, ver, st))
        expect_invalid(lib.eth_kzg_amd_verify_kzg_proof_many_device(None, 1, *args, ver, st, None))
