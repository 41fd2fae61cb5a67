"""csrc/verify_host.hpp: CellLeafTranscript -- the host statement of the cell verifier's leaf-hashed challenge -- on the CPU against
tests/leaf_transcript.py (hashlib).  No GPU: a stand-alone program (tests/c/test_leaf_transcript.cpp) built with hipcc's host pass, as
tests/test_host_units.py builds test_verify_host.cpp, once plain and once with AddressSanitizer + UBSan (its own main, run directly).

The transcript treats its inputs as opaque bytes, so seeded random bytes serve.  n = 1, 2 and 65 entries: every leaf digest, the root
and the reduced challenge; then that the root moves when two entries are exchanged and when one byte of any of the four fields changes
(the C++ and the hashlib roots are compared on each changed batch too, so "moves" is a statement about both)."""
import os
import random
import shutil
import subprocess

import pytest

import leaf_transcript as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def _batches():
    """-> {name: (commitments, indices, cells, proofs)}: a plain function of the seed"""
    rng = random.Random("leaf-transcript-host:1")
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))  # noqa: E731
    out = {}
    for n in (1, 2, 65):
        pool = [rb(48) for _ in range(3)]  # commitments repeat: the leaf takes the caller's bytes of entry k, whatever the rows are
        idx = [rng.randrange(128) for _ in range(n)]
        idx[0], idx[-1] = 0, 127 if n > 1 else 0
        out["n-%d" % n] = ([rng.choice(pool) for _ in range(n)], idx, [rb(2048) for _ in range(n)], [rb(48) for _ in range(n)])
    comm, idx, cells, proofs = out["n-65"]
    order = list(range(65))
    order[3], order[40] = order[40], order[3]
    out["exchanged"] = tuple([col[i] for i in order] for col in (comm, idx, cells, proofs))
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]  # noqa: E731
    out["commitment-byte"] = (comm[:17] + [flip(comm[17], 47)] + comm[18:], idx, cells, proofs)
    out["index"] = (comm, idx[:17] + [idx[17] ^ 1] + idx[18:], cells, proofs)
    out["cell-first-byte"] = (comm, idx, cells[:17] + [flip(cells[17], 0)] + cells[18:], proofs)
    out["cell-last-byte"] = (comm, idx, cells[:64] + [flip(cells[64], 2047)], proofs)
    out["proof-byte"] = (comm, idx, cells, [flip(proofs[0], 0)] + proofs[1:])
    return out


@pytest.fixture(scope="module")
def batches():
    return _batches()


@pytest.fixture(scope="module", params=list(BUILDS))
def printed(request, tmp_path_factory, batches):
    """-> {name: (leaf digests, root, r)} as one build of the program prints them"""
    tmp = tmp_path_factory.mktemp("leaf_transcript_" + request.param)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, cases = str(tmp / "test_leaf_transcript"), str(tmp / "cases.txt")
    subprocess.check_call([hipcc, *BUILDS[request.param], "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_leaf_transcript.cpp"), "-o", exe])
    with open(cases, "w") as f:
        for comm, idx, cells, proofs in batches.values():
            f.write("batch %d " % len(idx) + " ".join("%s %d %s %s" % (c.hex(), i, l.hex(), p.hex()) for c, i, l, p in zip(comm, idx, cells, proofs)) + "\n")
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(batches)
    out = {}
    for name, line in zip(batches, lines):
        word, leaves, root, r = line.split()
        assert word == "batch"
        out[name] = ([bytes.fromhex(x) for x in leaves.split(",")], bytes.fromhex(root), int(r, 16))
    return out


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["n-1", "n-2", "n-65"])
def test_leaves_root_and_challenge_match_hashlib(batches, printed, name):
    args = batches[name]
    leaves, root, r = printed[name]
    assert len(args[1]) == int(name[2:]) and args[1][0] == 0 and (len(args[1]) == 1 or args[1][-1] == 127)
    assert leaves == L.leaf_digests(*args)
    assert root == L.leaf_root(*args) == L.root_of(leaves)
    assert r == L.leaf_challenge(*args) == int.from_bytes(root, "big") % L.R


@pytest.mark.timeout(600)
def test_the_root_binds_the_order_and_every_field(batches, printed):
    base = printed["n-65"][1]
    seen = {base}
    for name in ("exchanged", "commitment-byte", "index", "cell-first-byte", "cell-last-byte", "proof-byte"):
        leaves, root, r = printed[name]
        assert root == L.leaf_root(*batches[name]) and leaves == L.leaf_digests(*batches[name]), name
        assert root not in seen, name
        seen.add(root)
    # an exchange moves exactly the two leaves that changed position (the position is hashed) and, through them, the root
    moved = [k for k in range(65) if printed["exchanged"][0][k] != printed["n-65"][0][k]]
    assert moved == [3, 40]
    # a changed field moves exactly its own leaf
    for name, k in (("commitment-byte", 17), ("index", 17), ("cell-first-byte", 17), ("cell-last-byte", 64), ("proof-byte", 0)):
        assert [j for j in range(65) if printed[name][0][j] != printed["n-65"][0][j]] == [k], name
