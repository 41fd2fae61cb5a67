"""Partial data columns (eth_kzg_amd_verify_partial_data_columns), on the CPU.

1. The case builder (tests/partial_columns.py): a partial call expands into the problems of the many-verification.
2. The HIP-free pieces csrc/verify_host.hpp gains for it -- validate_partial_columns_call, validate_partial_column (the stray-bit rule),
   PartialColumns, partial_column_view, vm_kept_partial_columns -- with the parts, chunks and copy runs over unequal columns and the
   per-column transcript digests and ROOTs, through a stand-alone program (tests/c/test_partial_columns.cpp, its own main) built with
   hipcc's host pass, once plain and once with AddressSanitizer + UBSan and run directly, against values written here from hashlib on the
   EXPANDED problems (tests/verify_transcript.py for the digests, tests/many_leaf.py for the ROOTs).  Nothing is loaded into Python under a sanitizer."""
import os
import random
import shutil
import subprocess

import pytest

import many_leaf as M
import partial_columns as P
import test_vm_plan_host as PLAN
import verify_transcript as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
BIG = 1 << 24
COMMITMENTS, INDICES, PRESENT, CELLS, PROOFS, VERIFIED = 1, 2, 4, 8, 16, 32  # the NULL bits of a `call` line

CALLS = [  # (name, flags, n_blobs, n_columns, NULL arrays, accepted): flags, then the column count, then NULL arrays
    ("plain", 0, 6, 128, 0, True),
    ("leaf-flag", 1, 6, 128, 0, True),
    ("stray-flag-bit", 2, 6, 128, 0, False),
    ("stray-flag-bit-next-to-the-leaf-flag", 3, 6, 128, 0, False),
    ("stray-flag-bit-in-an-empty-call", 0x80000000, 0, 0, 0, False),
    ("2^24-columns", 0, 1, BIG, 0, True),
    ("2^24+1-columns", 0, 1, BIG + 1, 0, False),
    ("2^24+1-columns-without-blobs", 0, 0, BIG + 1, 0, False),
    ("no-columns-and-no-arrays", 0, 6, 0, COMMITMENTS | INDICES | PRESENT | CELLS | PROOFS | VERIFIED, True),
    ("no-blobs-and-no-bitmaps-or-byte-arrays", 0, 0, 5, COMMITMENTS | PRESENT | CELLS | PROOFS, True),
    ("no-blobs-but-no-indices", 0, 0, 5, INDICES, False),
    ("no-blobs-but-no-verdicts", 0, 0, 5, VERIFIED, False),
    ("null-commitments", 0, 6, 5, COMMITMENTS, False),
    ("null-indices", 0, 6, 5, INDICES, False),
    ("null-bitmaps", 1, 6, 5, PRESENT, False),
    ("null-cells", 1, 6, 5, CELLS, False),
    ("null-proofs", 0, 6, 5, PROOFS, False),
    ("null-verdicts", 0, 6, 5, VERIFIED, False),
    ("too-many-blobs", 0, BIG, 5, 0, True),  # well-formed: every COLUMN is refused (status 3), below
    ("too-many-blobs-and-a-null-array", 0, BIG, 5, PRESENT, False),
]
SMALL = (2, 1, 3, 4)   # thresholds small enough for short lists to be cut: min_problems, min_cells, max_parts, chunk cells
ENGINE = (PLAN.MIN_PROBLEMS, PLAN.MIN_CELLS, PLAN.MAX_PARTS, PLAN.CHUNK)


def _plans():
    """(n_blobs, [(index, present)], thresholds): the word boundaries at 63, 64, 65 and 130 blobs, every kind of refusal, unequal columns"""
    full = lambda n: (1 << n) - 1  # noqa: E731
    out = []
    for nb in (63, 64, 65, 130):
        cols = [(0, full(nb)), (127, 1), (5, 1 << (nb - 1)), (128, 0), (1 << 40, 0), (128, 1), (7, 0),
                (9, 1 << nb), (9, full(nb) | 1 << nb), (9, 1 << (64 * P.words(nb) - 1)), (3, (1 << 62) | (1 << (nb - 1)) | 1)]
        if nb > 64:
            cols += [(11, 1 << 63), (12, 1 << 64), (13, (1 << 63) | (1 << 64)), (14, full(64)), (15, full(nb) ^ full(64))]
        cols = [c for c in cols if not c[1] >> (64 * P.words(nb))]  # (a bit beyond the W words cannot cross the ABI)
        out.append((nb, cols, SMALL))
    out.append((1, [(0, 1), (0, 0), (128, 1), (0, 2), (0, 3)], SMALL))
    out.append((0, [(0, 0), (500, 0), (127, 0)], SMALL))
    rng = random.Random("partial-columns-plans:1")
    for nb in (6, 70, 128):
        cols = [(rng.randrange(130), rng.getrandbits(nb) & rng.getrandbits(nb)) for _ in range(24)]
        out.append((nb, cols, SMALL))
    out.append((128, [(j % 128, (1 << (1 + j % 128)) - 1) for j in range(1025)], ENGINE))  # popcounts cycling 1..128: parts of the engine's size
    out.append((128, [(j % 128, (1 << (1 + j % 128)) - 1) for j in range(191)], ENGINE))   # below the problem threshold: chunks only
    return out


def _plan_line(nb, cols, thresholds):
    words = lambda p: " ".join("%x" % w for w in P.word_rows(nb, [p])[0])  # noqa: E731
    return "plan %d %d %d %d %d %d " % ((nb, len(cols)) + thresholds) + " ".join(("%d %s" % (i, words(p))).strip() for i, p in cols)


def _plan_want(nb, cols, thresholds):
    status = [P.validation_status(nb, i, p) for i, p in cols]
    m = [0 if s else len(P.blobs_of(nb, p)) for s, (_, p) in zip(status, cols)]
    start = [0]
    for _, p in cols:
        start.append(start[-1] + P.entries_of(nb, p))
    keep = [j for j, s in enumerate(status) if s == 0]
    kept = [m[j] for j in keep]
    parts = PLAN.parts_rule(kept, *thresholds[:3])
    chunks = PLAN.chunks_rule(kept, thresholds[3])
    runs = PLAN.runs_rule([(start[j], m[j], m[j] != 0) for j in keep])
    csv = lambda v: ",".join(str(x) for x in v)  # noqa: E731
    return "plan %s | %s | %s | %s | %s | %s | %s | 1" % (csv(status), csv(m), csv(start), csv(keep), csv(parts), csv(chunks),
                                                         ",".join("%d:%d:%d" % r for r in runs))


def _views():
    """(commitments as pool indices, present blobs): the order of a column's own list is that of ITS first occurrences"""
    return [([0, 1, 2], [0, 1, 2]), ([0, 1, 0], [1, 2]), ([0, 1, 0, 2], [2, 3]), ([0, 0, 0, 0], [1, 3]), ([0, 1, 2, 3, 4, 5], [5]),
            ([0, 1, 2, 1, 0, 2, 3], [6, 5, 4, 3][::-1]), ([3, 2, 1, 0, 0, 1, 2, 3], [4, 5, 6, 7]), ([0, 1], []),
            ([i % 7 for i in range(130)], list(range(60, 130, 3)))]


def _cases():
    """-> (lines of the case file, what each must print): a plain function of the seed"""
    rng = random.Random("partial-columns-host:1")
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))  # noqa: E731
    lines, want = [], []
    for _, flags, nb, nc, nulls, ok in CALLS:
        lines.append("call %d %d %d %d" % (flags, nb, nc, nulls))
        want.append("call %d" % (0 if ok else 3))
    for nb, cols, thresholds in _plans():
        lines.append(_plan_line(nb, cols, thresholds))
        want.append(_plan_want(nb, cols, thresholds))
    lines.append("plan %d 3 %d %d %d %d 0 127 128" % ((BIG,) + SMALL))  # too many blobs: every column 3, no bitmap read (none given)
    want.append("plan 3,3,3 | 0,0,0 | 0,0,0,0 |  | 0 | 0 |  | 1")
    for picks, held in _views():
        pool = [rb(48) for _ in range(max(picks) + 1)]
        comm = [pool[i] for i in picks]
        lines.append("view %d %s %d %s" % (len(comm), " ".join(c.hex() for c in comm), len(held), " ".join(str(b) for b in held)))
        uniq, row = T.dedup([comm[i] for i in held])  # the statement is about the EXPANDED problem
        pair_u, own, wide = P.pairs(comm, held)
        assert own == row and len(pair_u) == len(uniq) <= max(len(held), 0)
        csv = lambda v: ",".join(str(x) for x in v)  # noqa: E731
        want.append("view %s | %s | %s | %s | 1" % (",".join(u.hex() for u in uniq), csv(row), csv(wide), csv(pair_u)))
    shapes = [(3, [(0, 0b111), (127, 0b001), (64, 0b110)], [0, 1, 2]), (4, [(5, 0b1100), (5, 0b0011), (9, 0)], [0, 1, 0, 2]),
              (3, [(1, 0b110), (128, 0b1), (2, 0b1011), (1 << 40, 0)], [0, 1, 0]), (70, [(3, 1 << 63 | 1 << 64 | 1 << 69), (4, 1 << 70 | 1)], None)]
    for nb, cols, picks in shapes:
        pool = [rb(48) for _ in range(nb)]
        comm = [pool[i] for i in picks] if picks else pool
        present = [p for _, p in cols]
        m = [len(P.blobs_of(nb, p)) for p in present]
        call = (comm, [i for i, _ in cols], present, [[rb(2048) for _ in range(k)] for k in m], [[rb(48) for _ in range(k)] for k in m])
        flat = P.flat_bytes(call)
        words = lambda p: " ".join("%x" % w for w in P.word_rows(nb, [p])[0])  # noqa: E731
        lines.append(("digests %d %d " % (nb, len(cols)) + " ".join("%d %s" % (i, words(p)) for i, p in cols) + " " +
                      " ".join(f.hex() for f in flat if f)))
        want.append("digests " + ",".join("-" if a is None else "%s:%s" % (T.cell_digest(*a).hex(), M.problem_root(a).hex()) for a in P.expand(*call)))
    return lines, want


def test_a_partial_call_expands_into_problems_of_the_many_verification(printed):
    """the statement module against itself, and against what the stand-alone program printed for the same shapes"""
    plain = [l for l in printed[0] if l.startswith("view 3 ")][1]  # blobs X Y X, blobs 1 and 2 present
    got = printed[2][printed[0].index(plain)].split(" | ")
    assert got[1:] == ["0,1", "1,0", "1,0", "1"]  # own rows, pass-wide rows, pair_u: the list is Y X, as P.pairs says below
    comm = ["c0", "c1", "c0", "c3"]
    call = P.mask((comm, [127, 3, 9], [["a0", "a1", "a2", "a3"], ["b0", "b1", "b2", "b3"], ["x0", "x1", "x2", "x3"]],
                   [["p0", "p1", "p2", "p3"], ["q0", "q1", "q2", "q3"], ["y0", "y1", "y2", "y3"]]), [0b1100, 0b0001, 0])
    assert call[3] == [["a2", "a3"], ["b0"], []] and call[4] == [["p2", "p3"], ["q0"], []]
    assert P.expand(*call) == [(["c0", "c3"], [127, 127], ["a2", "a3"], ["p2", "p3"]), (["c1"] * 0 + ["c0"], [3], ["b0"], ["q0"]), ([], [], [], [])]
    # statuses: the bound first, then stray bits, then an index that is read only where the column holds a cell
    table = [(6, 0, 0b111111, 0), (6, 0, 0b1000000, 3), (6, 128, 0, 0), (6, 128, 1, 3), (6, 1 << 40, 0, 0), (0, 500, 0, 0), (0, 0, 1, 3),
             (63, 0, 1 << 62, 0), (63, 0, 1 << 63, 3), (64, 0, 1 << 63, 0), (64, 0, 1 << 64, 3), (65, 0, 1 << 64, 0), (65, 0, 1 << 65, 3),
             (130, 0, 1 << 129, 0), (130, 0, 1 << 130, 3), (130, 0, 1 << 191, 3), (BIG - 1, 0, 1, 0), (BIG, 0, 0, 3), (BIG, 0, 1, 3)]
    assert [P.validation_status(nb, i, p) for nb, i, p, _ in table] == [s for *_, s in table]
    assert P.expand(comm, [0, 200], [0b10000, 1], [[], ["a"]], [[], ["p"]]) == [None, None]
    # a refused column keeps the entries of ALL its set bits in the packed arrays; the words of the ABI
    assert [P.entries_of(70, p) for p in (1 << 69, 1 << 70, (1 << 127) | 3, 1 << 128)] == [1, 1, 3, 0]
    assert P.word_rows(70, [(1 << 69) | (1 << 63) | 1]) == [[(1 << 63) | 1, 1 << 5]] and P.word_rows(0, [0, 0]) == [[], []]
    assert P.flat_bytes(([b"C"], [0, 0], [0b11, 0b1], [[b"a"], [b"b"]], [[b"p"], [b"q"]]), filler=b"") == (b"C", b"ab", b"pq")
    # blobs X Y X: the column that holds blobs 1 and 2 names Y first -- its own list is NOT in the order of the call's
    assert P.pairs(["X", "Y", "X"], [1, 2]) == ([1, 0], [0, 1], [1, 0]) and P.dedup(["Y", "X"]) == (["Y", "X"], [0, 1])
    assert P.pairs(["X", "Y", "X", "Z"], [2, 3]) == ([0, 2], [0, 1], [0, 2])
    # 129 columns x 130 different blobs with one cell each: 129 + 129 + 129, not 129 + 129 * 130 + 129
    comm = ["c%d" % i for i in range(130)]
    assert P.counts(comm, list(range(128)) + [0], [1 << j for j in range(129)]) == (130, 129 * 3)
    assert P.counts(["X", "Y", "X"], [0, 1], [0b111, 0b101]) == (2, 5 + 3 + 2)
    import data_columns as D
    assert D.counts(129, 129, 130) == (130, 129 + 129 * 130 + 129)  # what the dense addressing would launch for that shape


@pytest.fixture(scope="module", params=list(BUILDS))
def printed(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("partial_columns_" + request.param)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, cases = str(tmp / "test_partial_columns"), str(tmp / "cases.txt")
    subprocess.check_call([hipcc, *BUILDS[request.param], "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_partial_columns.cpp"), "-o", exe])
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
    assert {"stray-flag-bit-in-an-empty-call", "2^24+1-columns", "null-bitmaps", "no-blobs-and-no-bitmaps-or-byte-arrays"} <= {c[0] for c in CALLS}


@pytest.mark.timeout(600)
def test_stray_bits_word_boundaries_entry_counts_and_cuts_over_unequal_columns(printed):
    plans = _plans()
    for l, g, w in _rows(printed, "plan", len(plans) + 1):
        assert g == w, (l[:60], g[:300], w[:300])
    assert {nb for nb, _, _ in plans} >= {63, 64, 65, 130, 0}
    # the engine-size list is really cut into three parts and two chunks, at column boundaries, and its columns are unequal
    kept = [1 + j % 128 for j in range(1025)]
    parts, chunks = PLAN.parts_rule(kept, *ENGINE[:3]), PLAN.chunks_rule(kept, ENGINE[3])
    assert len(parts) == 4 and len(chunks) >= 2 and sum(kept) < PLAN.CHUNK  # (66 k cells: one chunk per part, three parts)
    assert len(PLAN.chunks_rule([128] * 1025, ENGINE[3])) == 3


@pytest.mark.timeout(600)
def test_a_columns_own_list_rows_and_pairs_equal_the_expanded_problems(printed):
    for l, g, w in _rows(printed, "view", len(_views())):
        assert g == w, (l[-60:], g[-200:], w[-200:])
        assert g.endswith("| 1")  # the program's own comparison with dedup_commitments of the expanded problem, and P <= m


@pytest.mark.timeout(600)
def test_partial_column_digests_and_roots_equal_the_expanded_problems(printed):
    for l, g, w in _rows(printed, "digests", 4):
        assert g == w, l[:40]
