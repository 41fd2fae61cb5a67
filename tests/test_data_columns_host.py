"""The data columns of one block (eth_kzg_amd_verify_data_columns), on the CPU.

1. The case builder (tests/data_columns.py): a column call expands into the problems of the many-verification.
2. The HIP-free pieces csrc/verify_host.hpp gains for it -- validate_data_columns_call, validate_data_column, ColumnCommitments -- and
   the per-column transcript digests and ROOTs taken over the call's ONE de-duplicated list, through a stand-alone program
   (tests/c/test_data_columns.cpp, its own main) built with hipcc's host pass, once plain and once with AddressSanitizer + UBSan and run
   directly, against values written here from hashlib on the EXPANDED problems.  Nothing is loaded into Python under a sanitizer."""
import os
import random
import shutil
import subprocess

import pytest

import data_columns as D
import leaf_transcript as L
import verify_transcript as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
BIG = 1 << 24
COMMITMENTS, INDICES, CELLS, PROOFS, VERIFIED = 1, 2, 4, 8, 16  # the NULL bits of a `call` line

CALLS = [  # (name, flags, n_blobs, n_columns, NULL arrays, accepted)
    ("plain", 0, 6, 128, 0, True),
    ("leaf-flag", 1, 6, 128, 0, True),
    ("stray-flag-bit", 2, 6, 128, 0, False),
    ("stray-flag-bit-next-to-the-leaf-flag", 3, 6, 128, 0, False),
    ("stray-flag-bit-in-an-empty-call", 0x80000000, 0, 0, 0, False),
    ("2^24-columns", 0, 1, BIG, 0, True),
    ("2^24+1-columns", 0, 1, BIG + 1, 0, False),
    ("2^24+1-columns-without-blobs", 0, 0, BIG + 1, 0, False),
    ("no-columns-and-no-arrays", 0, 6, 0, COMMITMENTS | INDICES | CELLS | PROOFS | VERIFIED, True),
    ("no-blobs-and-no-byte-arrays", 0, 0, 5, COMMITMENTS | CELLS | PROOFS, True),
    ("no-blobs-but-no-indices", 0, 0, 5, INDICES, False),
    ("no-blobs-but-no-verdicts", 0, 0, 5, VERIFIED, False),
    ("null-commitments", 0, 6, 5, COMMITMENTS, False),
    ("null-indices", 0, 6, 5, INDICES, False),
    ("null-cells", 1, 6, 5, CELLS, False),
    ("null-proofs", 0, 6, 5, PROOFS, False),
    ("null-verdicts", 0, 6, 5, VERIFIED, False),
    ("too-many-blobs", 0, BIG, 5, 0, True),  # well-formed: every COLUMN is refused (status 3), below
    ("too-many-blobs-and-a-null-array", 0, BIG, 5, CELLS, False),  # a NULL array with a non-zero count, whatever the count
]
COLUMNS = [(1, 0), (1, 127), (1, 128), (6, 127), (6, 128), (6, 1 << 63), (0, 0), (0, 128), (0, 1 << 40), (4096, 127), (4096, 128),
           (BIG - 1, 127), (BIG - 1, 128), (BIG, 0), (BIG + 7, 5), (1 << 40, 0)]


def test_a_column_call_expands_into_problems_of_the_many_verification():
    comm = ["c0", "c1", "c0"]
    cells, proofs = [["a0", "a1", "a2"], ["b0", "b1", "b2"]], [["p0", "p1", "p2"], ["q0", "q1", "q2"]]
    assert D.expand(comm, [127, 3], cells, proofs) == [(comm, [127] * 3, cells[0], proofs[0]), (comm, [3] * 3, cells[1], proofs[1])]
    assert D.expand([], [5, 500], [[], []], [[], []]) == [([], [], [], []), ([], [], [], [])]  # no blobs: empty problems, the index unread
    assert D.expand(comm, [], [], []) == []
    assert [D.validation_status(n, c) for n, c in COLUMNS] == [0, 0, 3, 0, 3, 3, 0, 0, 0, 0, 3, 0, 3, 3, 3, 3]
    mat_cells = [["%d.%d" % (b, c) for c in range(128)] for b in range(2)]
    blk = D.block(["C0", "C1"], mat_cells, mat_cells, [1, 0, 1], [127, 128, 0])
    assert blk[0] == ["C1", "C0", "C1"] and blk[2][0] == ["1.127", "0.127", "1.127"] and blk[2][1] == blk[2][2] == ["1.0", "0.0", "1.0"]
    assert D.flat_bytes([b"ab", b"cd"], [[b"1", b"2"], [b"3", b"4"]], [[b"w", b"x"], [b"y", b"z"]]) == (b"abcd", b"1234", b"wxyz")
    # the multiplications of a pass of 128 columns x 64 different blobs against the expanded pass's: the count behind "three of five"
    n = 128 * 64
    assert D.counts(n, 128, 64) == (64, n + n + 128) and 2 * n + 128 * 64 == 3 * n


def _cases():
    """-> (lines of the case file, what each must print): a plain function of the seed"""
    rng = random.Random("data-columns-host:1")
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))  # noqa: E731
    lines, want = [], []
    for _, flags, nb, nc, nulls, ok in CALLS:
        lines.append("call %d %d %d %d" % (flags, nb, nc, nulls))
        want.append("call %d" % (0 if ok else 3))
    for nb, index in COLUMNS:
        lines.append("column %d %d" % (nb, index))
        want.append("column %d 1" % D.validation_status(nb, index))
    for nc, n, pool_size in ((1, 1, 1), (3, 2, 1), (4, 7, 3), (2, 130, 4), (128, 64, 64), (3, 65, 64)):
        pool = [rb(48) for _ in range(pool_size)]
        comm = [pool[i] if i < pool_size else rng.choice(pool) for i in range(n)]
        rng.shuffle(comm)
        uniq, row = T.dedup(comm)
        lines.append("dedup %d %d " % (nc, n) + " ".join(c.hex() for c in comm))
        want.append("dedup %d %s %s 1" % (len(uniq), ",".join(str(r) for r in row), ",".join(u.hex() for u in uniq)))
    for nb, indices, pool_size in ((1, [0], 1), (3, [127, 0, 127], 2), (5, [1, 64], 5), (4, [9], 1)):
        pool = [rb(48) for _ in range(pool_size)]
        comm = [pool[i % pool_size] for i in range(nb)]
        rng.shuffle(comm)
        cells = [[rb(2048) for _ in range(nb)] for _ in indices]
        proofs = [[rb(48) for _ in range(nb)] for _ in indices]
        flat = D.flat_bytes(comm, cells, proofs)
        lines.append("digests %d %d %s %s %s %s" % (nb, len(indices), " ".join(str(i) for i in indices), flat[0].hex(), flat[1].hex(), flat[2].hex()))
        problems = D.expand(comm, indices, cells, proofs)  # the statement is about the EXPANDED problems
        want.append("digests " + ",".join("%s:%s" % (T.cell_digest(*a).hex(), L.leaf_root(*a).hex()) for a in problems))
    return lines, want


@pytest.fixture(scope="module", params=list(BUILDS))
def printed(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("data_columns_" + request.param)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, cases = str(tmp / "test_data_columns"), str(tmp / "cases.txt")
    subprocess.check_call([hipcc, *BUILDS[request.param], "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_data_columns.cpp"), "-o", exe])
    lines, want = _cases()
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    return lines, want, got


def _rows(printed, command, count):
    lines, want, got = printed
    rows = [(l, g, w) for l, g, w in zip(lines, got, want) if l.split()[0] == command]
    assert len(rows) == count
    return rows


@pytest.mark.timeout(600)
def test_call_level_validation_order_and_bounds(printed):
    rows = _rows(printed, "call", len(CALLS))
    for (name, *_), (l, g, w) in zip(CALLS, rows):
        assert g == w, (name, l, g)
    names = {c[0] for c in CALLS}
    assert {"stray-flag-bit-in-an-empty-call", "2^24-columns", "2^24+1-columns", "no-blobs-and-no-byte-arrays", "null-cells"} <= names


@pytest.mark.timeout(600)
def test_a_column_is_validated_as_its_expanded_problem(printed):
    for (nb, index), (l, g, w) in zip(COLUMNS, _rows(printed, "column", len(COLUMNS))):
        assert g == w, (l, g)  # the status, and the program's own comparison with validate_cell_batch of the expanded problem
    assert (BIG - 1, 127) in COLUMNS and (BIG, 0) in COLUMNS and (0, 128) in COLUMNS  # the bound is 2^24 - 1; no blobs: the index is unread


@pytest.mark.timeout(600)
def test_one_deduplication_per_call_equals_one_per_column(printed):
    for l, g, w in _rows(printed, "dedup", 6):
        assert g == w, l[:40]
        assert g.endswith(" 1")  # list form == flat form == every column's own run


@pytest.mark.timeout(600)
def test_column_digests_and_roots_equal_the_expanded_problems(printed):
    for l, g, w in _rows(printed, "digests", 4):
        assert g == w, l[:40]
