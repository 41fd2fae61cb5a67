"""k_pairing_check (csrc/k_pairing.hip) through the hook eth_kzg_amd_test_pairing_check_many: many pairing checks per launch, one per lane.

Ground truth comes BY CONSTRUCTION, independent of the code under test.  S_i = [tau^i]_1 are the setup's monomial G1 points, the keys are
key 0 = ([tau^64]_2, -[1]_2) with k = 64 and key 1 = ([tau]_2, -[1]_2) with k = 1, and a S comes from the CPU oracle's oracle_g1_mul:
  (a S_i, a S_(i+k)) passes;  (a S_i, b S_(i+k)) with b != a, the swapped pair and (a S_i, -a S_(i+k)) fail;
  (O, O) passes;  (O, X) and (X, O) fail.
Counts 1, 2, 63, 64, 65, 129 -- the wave edges and the padding lanes --, valid and wrong entries interleaved so that neighbours differ,
both keys, normalised points and points multiplied through by a Z of their own.  The kernel's verdicts equal the construction and the
host threads'; with normalised points its Miller values equal the host's byte for byte; a poisoned slot gives -1 for that entry only."""
import ctypes as C
import hashlib
import importlib
import os

import pytest

import oracle_lib
import synth

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu
R = synth.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETUP = os.path.join(ROOT, "rust-eth-kzg_amd", "data", "trusted_setup_4096.bin")
INF = b"\xc0" + bytes(47)
COUNTS = [1, 2, 63, 64, 65, 129]
_cache = {}  # the oracle's multiples: computed once, shared by the tests, never changed


def _ctx(**env):
    import torch
    torch.cuda.init()
    env = dict(env, ETH_KZG_AMD_TABLE_GB="3")  # the start tables: nothing here depends on the table
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return kzg.DASContext(use_precomp=True)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    c = _ctx()
    yield c
    c.close()


def setup_point(i):
    if "srs" not in _cache:
        with open(SETUP, "rb") as f:
            _cache["srs"] = f.read()
    return _cache["srs"][16 + 48 * i:16 + 48 * i + 48]


def scalar(tag):
    return int.from_bytes(hashlib.sha256(b"pairing-many:" + tag).digest(), "big") % R


def multiple(i, k):
    if (i, k) not in _cache:
        _cache[(i, k)] = oracle_lib.g1_mul(setup_point(i), k.to_bytes(32, "big"))
    return _cache[(i, k)]


def negated(p):
    assert p != INF
    return bytes([p[0] ^ 0x20]) + p[1:]


# (name, verdict); the order interleaves valid and wrong entries: no two neighbours agree, also across the end of the list
CASES = [("valid", 1), ("other_scalar", 0), ("O_O", 1), ("swapped", 0), ("valid", 1), ("negated", 0), ("valid", 1), ("O_X", 0), ("O_O", 1),
         ("X_O", 0)]


def entries(key, n):
    """n pairs and their verdicts by construction; entry e takes case e mod 10 at a position and with scalars of its own class"""
    k = 64 if key == 0 else 1
    pairs, want = [], []
    for e in range(n):
        name, verdict = CASES[e % len(CASES)]
        i = (0, 4095 - k, 1, 2047, 100)[e % 5]  # both ends of the setup and three places between
        a, b = scalar(b"a%d" % (e % 3)), scalar(b"b%d" % (e % 3))
        p, q = multiple(i, a), multiple(i + k, a)
        pair = {"valid": (p, q), "other_scalar": (p, multiple(i + k, b)), "swapped": (q, p), "negated": (p, negated(q)), "O_O": (INF, INF),
                "O_X": (INF, q), "X_O": (p, INF)}[name]
        pairs.append(pair[0] + pair[1])
        want.append(verdict)
    assert all(want[e] != want[e + 1] for e in range(n - 1))
    return b"".join(pairs), want


def check_many(ctx, key, n, pairs, flags, millers=True):
    lib = kzg.load_library()
    gpu, host = (C.c_int8 * n)(), (C.c_int8 * n)()
    mg, mh = (C.create_string_buffer(576 * n), C.create_string_buffer(576 * n)) if millers else (None, None)
    rc = lib.eth_kzg_amd_test_pairing_check_many(ctx.handle, key, n, pairs, flags, gpu, host, mg, mh)
    assert rc == 0, rc
    return list(gpu), list(host), mg.raw if millers else None, mh.raw if millers else None


@pytest.mark.parametrize("rescale", [0, 1])
@pytest.mark.parametrize("key", [0, 1])
@pytest.mark.parametrize("n", COUNTS)
def test_verdicts_by_construction(ctx, n, key, rescale):
    pairs, want = entries(key, n)
    gpu, host, mg, mh = check_many(ctx, key, n, pairs, rescale)
    print("n", n, "key", key, "rescale", rescale, "gpu", gpu[:12], "host", host[:12], "want", want[:12])
    assert gpu == want
    assert gpu == host
    if not rescale:  # affine inputs: the same operations in the same order on both sides
        for e in range(n):
            assert mg[576 * e:576 * e + 576] == mh[576 * e:576 * e + 576], e
    one = mg[576 * 2:576 * 3] if n > 2 else None  # entry 2 is (O, O): its Miller value is 1, with nothing after the first 48 bytes
    assert one is None or (one == mh[576 * 2:576 * 3] and one[48:] == bytes(528) and one[:48] != bytes(48))


@pytest.mark.parametrize("key", [0, 1])
def test_a_poisoned_slot_gives_minus_one_for_that_entry_only(ctx, key):
    n, e = 65, 64  # the entry alone in the second wave, in front of 63 padding lanes
    pairs, want = entries(key, n)
    gpu, host, _, _ = check_many(ctx, key, n, pairs, 2 | (e << 8), millers=False)
    want[e] = -1
    assert gpu == want and host == want
    gpu, host, _, _ = check_many(ctx, key, n, pairs, 2 | (3 << 8), millers=False)  # and inside a full wave
    want[e], want[3] = CASES[e % len(CASES)][1], -1
    assert gpu == want and host == want


def test_the_hook_refuses_what_it_cannot_run(ctx):
    lib = kzg.load_library()
    pairs, _ = entries(0, 1)
    out = (C.c_int8 * 1)()
    assert lib.eth_kzg_amd_test_pairing_check_many(ctx.handle, 2, 1, pairs, 0, out, out, None, None) == 3
    assert lib.eth_kzg_amd_test_pairing_check_many(ctx.handle, 0, 0, pairs, 0, out, out, None, None) == 3
    assert lib.eth_kzg_amd_test_pairing_check_many(ctx.handle, 0, 1, pairs, 2 | (1 << 8), out, out, None, None) == 3  # no such entry
    assert lib.eth_kzg_amd_test_pairing_check_many(ctx.handle, 0, 1, bytes(96), 0, out, out, None, None) == 2  # not a compressed point
