"""The many-verification with leaf-hashed challenges, on the CPU.

1. The statement (tests/many_leaf.py) on verify_transcript.many_cases(), with the oracle's cells and proofs as material: the leaves of
   a problem hash positions that restart at 0, a problem that is empty or refused at validation has a zero digest, and changing one
   byte of one cell changes that problem's root and EVERY weight of its pass (the fold seed hashes every root).
2. The pieces csrc/verify_host.hpp gains for it -- validate_cell_starts, dedup_commitments_flat, cell_leaf_root -- through a stand-alone
   program (tests/c/test_many_leaf.cpp, its own main) built with hipcc's host pass, once plain and once with AddressSanitizer + UBSan and
   run directly, against values written here from hashlib.  Nothing is loaded into Python under a sanitizer."""
import os
import random
import shutil
import subprocess

import pytest

import leaf_transcript as L
import many_leaf as M
import verify_transcript as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
MANY_PASSES = {p.name: p for p in T.many_cases()}


# ---- 1. the statement ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def material(oracle):
    blobs = T.material_blobs()
    cp = [oracle.compute_cells_and_kzg_proofs(b) for b in blobs]
    comms = [oracle.blob_to_kzg_commitment(b) for b in blobs]
    return T.Material(blobs, comms, [c for c, _ in cp], [p for _, p in cp], [None] * len(blobs))


@pytest.mark.parametrize("name", list(MANY_PASSES))
def test_positions_restart_and_unhashed_problems_have_zero_digests(material, name):
    p = MANY_PASSES[name]
    problems = [q.args(material) for q in p.problems]
    hashed = [q.kind not in ("empty", "bad-index") for q in p.problems]
    assert hashed == [q.hashed for q in p.problems]
    digests = M.pass_digests(problems, hashed)
    for b, (q, a) in enumerate(zip(p.problems, problems)):
        if not hashed[b]:
            assert digests[b] == bytes(32), (name, b)
            continue
        comm, idx, cells, proofs = a
        leaves = M.problem_leaves(a)
        # the first leaf of every problem hashes position 0, whatever stands in front of the problem in the pass
        assert leaves[0] == L.leaf_digest(0, idx[0], comm[0], proofs[0], cells[0]), (name, b)
        assert leaves[-1] == L.leaf_digest(len(idx) - 1, idx[-1], comm[-1], proofs[-1], cells[-1]), (name, b)
        # exactly the single flagged call's challenge for the problem alone: the root carries the problem's own n
        assert digests[b] == L.leaf_root(*a) == L.root_of(leaves) != bytes(32), (name, b)
    # the same through the flat form: the leaves of the call back to back, cut at cell_starts
    flat = M.pass_leaves(problems, hashed)
    starts = M.flat_arrays(problems)[0]
    assert len(flat) == starts[-1] and len(starts) == len(problems) + 1
    for b in range(len(problems)):
        if hashed[b]:
            assert L.root_of(flat[starts[b]:starts[b + 1]]) == digests[b], (name, b)
        else:
            assert set(flat[starts[b]:starts[b + 1]]) <= {bytes(32)}, (name, b)


@pytest.mark.parametrize("name", ["short-holes", "large-folded", "large-one-live", "search"])
def test_one_byte_of_one_cell_moves_its_root_and_every_weight(material, name):
    p = MANY_PASSES[name]
    problems = [q.args(material) for q in p.problems]
    hashed, live = [q.hashed for q in p.problems], [q.live for q in p.problems]
    digests = M.pass_digests(problems, hashed)
    rho = T.fold_weights(digests, live)
    assert [r != 0 for r in rho] == live and len({r for r in rho if r}) == sum(live)
    victim = max(b for b in range(len(problems)) if live[b])
    comm, idx, cells, proofs = problems[victim]
    k = len(cells) // 2
    changed = list(problems)
    changed[victim] = (comm, idx, cells[:k] + [cells[k][:100] + bytes([cells[k][100] ^ 1]) + cells[k][101:]] + cells[k + 1:], proofs)
    digests2 = M.pass_digests(changed, hashed)
    assert [b for b in range(len(problems)) if digests2[b] != digests[b]] == [victim], name
    rho2 = T.fold_weights(digests2, live)
    assert all(a != b for a, b, on in zip(rho, rho2, live) if on) and [r != 0 for r in rho2] == live, name
    # and the weights are not the reference transcript's
    ref = T.fold_weights([T.cell_digest(*a) if on else bytes(32) for a, on in zip(problems, hashed)], live)
    assert all(a != b for a, b, on in zip(rho, ref, live) if on), name


def test_the_flat_builder():
    a = (["c0", "c1"], [5, 6], ["l0", "l1"], ["p0", "p1"])
    b = ([], [], [], [])
    c = (["c2"], [7], ["l2"], ["p2"])
    assert M.flat_arrays([b, a, b, c, b]) == ([0, 0, 2, 2, 3, 3], ["c0", "c1", "c2"], [5, 6, 7], ["l0", "l1", "l2"], ["p0", "p1", "p2"])
    assert M.flat_arrays([]) == ([0], [], [], [], [])


# ---- 2. csrc/verify_host.hpp through a stand-alone program ------------------------------------------------------------------------------------
BIG = 1 << 24
STARTS = [  # (name, n_batches, entries or None for a NULL pointer, accepted)
    ("empty-call", 0, [], True),
    ("one-problem", 1, [0, 5], True),
    ("zero-length-first", 3, [0, 0, 4, 9], True),
    ("zero-length-middle", 3, [0, 4, 4, 9], True),
    ("zero-length-last", 3, [0, 4, 9, 9], True),
    ("only-empty-problems", 4, [0, 0, 0, 0, 0], True),
    ("decreasing", 3, [0, 4, 3, 9], False),
    ("decreasing-at-the-end", 2, [0, 4, 3], False),
    ("first-not-zero", 2, [1, 4, 9], False),
    ("null-with-problems", 2, None, False),
    ("a-problem-of-2^24-cells", 2, [0, BIG, BIG + 3], True),  # well-formed: the PROBLEM is refused (status 3), below
]


def _cases():
    """-> (lines of the case file, what each must print): a plain function of the seed"""
    rng = random.Random("many-leaf-host:1")
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))  # noqa: E731
    lines, want = [], []
    for _, nb, entries, ok in STARTS:
        lines.append("starts-null %d" % nb if entries is None else ("starts %d " % nb + " ".join(str(v) for v in entries)).strip())
        want.append("starts %d" % (0 if ok else 3))
    for n, status in ((0, 0), (BIG, 3), (BIG + 3, 3)):  # the bound is 2^24 - 1 cells
        lines.append("size %d" % n)
        want.append("size %d" % status)
    for n, pool_size in ((1, 1), (2, 1), (7, 3), (130, 4), (64, 64)):
        pool = [rb(48) for _ in range(pool_size)]
        comm = [pool[i] if i < pool_size else rng.choice(pool) for i in range(n)]
        rng.shuffle(comm)
        uniq, row = T.dedup(comm)
        lines.append("dedup %d " % n + " ".join(c.hex() for c in comm))
        want.append("dedup %d %s %s 1" % (len(uniq), ",".join(str(r) for r in row), ",".join(u.hex() for u in uniq)))
    for starts in ([0, 1], [0, 1, 64, 128, 193, 195, 195, 198, 326], [0, 0, 2, 2], [5, 6, 6, 9], [0, 0, 0]):
        leaves = [rb(32) for _ in range(starts[-1] - starts[0])]
        lines.append("roots %d %s %s" % (len(starts) - 1, " ".join(str(v) for v in starts), b"".join(leaves).hex() or "-"))
        roots = [L.root_of(leaves[lo - starts[0]:hi - starts[0]]) for lo, hi in zip(starts, starts[1:])]
        want.append("roots " + ",".join("%s:%064x" % (d.hex(), int.from_bytes(d, "big") % L.R) for d in roots))
    return lines, want


@pytest.fixture(scope="module", params=list(BUILDS))
def printed(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("many_leaf_" + request.param)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, cases = str(tmp / "test_many_leaf"), str(tmp / "cases.txt")
    subprocess.check_call([hipcc, *BUILDS[request.param], "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_many_leaf.cpp"), "-o", exe])
    lines, want = _cases()
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    return lines, want, got


@pytest.mark.timeout(600)
def test_cell_starts_are_accepted_or_refused(printed):
    lines, want, got = printed
    names = [s[0] for s in STARTS]
    assert names[:6] == ["empty-call", "one-problem", "zero-length-first", "zero-length-middle", "zero-length-last", "only-empty-problems"]
    assert {"decreasing", "first-not-zero", "null-with-problems", "a-problem-of-2^24-cells"} <= set(names)
    for i, name in enumerate(names):
        assert got[i] == want[i], (name, lines[i], got[i])
    sizes = [(l, g, w) for l, g, w in zip(lines, got, want) if l.startswith("size")]
    assert len(sizes) == 3 and all(g == w for _, g, w in sizes), sizes
    assert ("size %d" % BIG, "size 3", "size 3") in sizes  # a problem of 2^24 cells: its cell_starts are accepted, the problem is not


@pytest.mark.timeout(600)
def test_flat_deduplication_equals_the_pointer_list_form(printed):
    lines, want, got = printed
    rows = [(l, g, w) for l, g, w in zip(lines, got, want) if l.startswith("dedup")]
    assert len(rows) == 5
    for l, g, w in rows:
        assert g == w, l[:40]
        assert g.endswith(" 1")  # the program's own comparison of the two forms, and that the flat form points into the flat bytes


@pytest.mark.timeout(600)
def test_roots_per_problem_equal_hashlib(printed):
    lines, want, got = printed
    rows = [(l, g, w) for l, g, w in zip(lines, got, want) if l.startswith("roots")]
    assert len(rows) == 5
    for l, g, w in rows:
        assert g == w, l[:60]
