"""The bookkeeping of the cell many-verification (csrc/verify_many.hip), on the CPU: the cut of a call into parts, of a part into
chunks, the coalescing of problems into copy runs, the columns a column call keeps.

The four are HIP-free functions of csrc/verify_host.hpp (vm_call_parts, vm_chunk_end, vm_copy_runs, vm_kept_columns), run through a
stand-alone program (tests/c/test_vm_plan.cpp, its own main) built with hipcc's host pass, once plain and once with AddressSanitizer +
UBSan, and run directly.  Nothing is loaded into Python under a sanitizer.  What each must print is worked out here from a statement of
the rule that shares no code and no loop shape with the C++, and the properties the pass relies on are asserted on the output itself."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

import data_columns as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
MIN_PROBLEMS, MIN_CELLS, MAX_PARTS, CHUNK = 192, 24576, 3, 131072  # engine.hpp; test_the_constants_are_the_engines
BIG = 1 << 24


# ---- the rules, restated
def parts_rule(cells, min_problems, min_cells, max_parts):
    """Cut k of max_parts lies behind the first problem, after cut k - 1 and not the last, with which the running total reaches k
    shares of the total; a call below either threshold is not cut."""
    B, total = len(cells), sum(cells)
    if B == 0:
        return [0]
    cuts = [0]
    if max_parts > 1 and B >= min_problems and total >= min_cells:
        prefix = list(itertools.accumulate(cells))
        for k in range(1, max_parts):
            where = [j for j in range(cuts[-1] + 1, B) if prefix[j - 1] * max_parts >= k * total]
            if not where:
                break
            cuts.append(where[0])
    return cuts + [B]


def chunks_rule(n, limit):
    """From its first problem a chunk takes the longest stretch whose cells stay within the limit, and one problem at the least."""
    ends, before = [0], [0] + list(itertools.accumulate(n))  # (no count is negative: a stretch that fits holds only stretches that fit)
    while ends[-1] < len(n):
        b0 = ends[-1]
        fits = [e for e in range(b0 + 1, len(n) + 1) if before[e] - before[b0] <= limit]
        ends.append(max(fits) if fits else b0 + 1)
    return ends


def entries(problems):
    """-> the source entry of every destination entry: the entries of the problems that take part, in order"""
    return [src + j for src, length, takes in problems if takes for j in range(length)]


def runs_rule(problems):
    """Entry by entry: a new run wherever the source entry is not the one behind the entry before."""
    runs = []
    for dst, src in enumerate(entries(problems)):
        if runs and runs[-1][0] + runs[-1][1] == src:
            runs[-1][1] += 1
        else:
            runs.append([src, 1, dst])
    return [tuple(r) for r in runs]


def laid_out(sizes, skipped=()):
    """problems that follow each other in the source (cell_starts), those of `skipped` taking no part"""
    starts = [0] + list(itertools.accumulate(sizes))
    return [(starts[i], s, 0 if i in skipped else 1) for i, s in enumerate(sizes)]


PARTS = [  # (name, cells)
    ("B=0", []),
    ("B=1", [70000]),
    ("B=191-many-cells", [200] * 191),
    ("B=192-24575-cells", [128] * 191 + [127]),
    ("B=192-24576-cells", [128] * 192),
    ("B=193", [128] * 193),
    ("B=193-24575-cells", [127] * 192 + [24575 - 127 * 192]),
    ("one-problem-above-two-thirds-first", [100000] + [100] * 199),
    ("one-problem-above-two-thirds-middle", [100] * 100 + [100000] + [100] * 99),
    ("one-problem-above-two-thirds-last", [100] * 199 + [100000]),
    ("everything-in-the-last-problem", [0] * 199 + [30000]),
    ("three-equal-problems", [128, 128, 128]),
    ("empty-problems-between", [0, 300, 0, 0, 300, 0, 300] * 30),
    ("1024-of-128", [128] * 1024),
    ("uneven", [(7 * i) % 251 + 1 for i in range(500)]),
]
LOW_THRESHOLDS = [("three-equal-problems", [5, 5, 5]), ("two-problems", [1, 9]), ("one-problem", [4]), ("four-equal", [2, 2, 2, 2]),
                  ("zeros", [0, 0, 0, 0])]  # with thresholds of 1 problem and 1 cell: the cut itself at sizes a reader can check by hand
CHUNKS = [  # (name, cells per problem)
    ("none", []),
    ("one", [5]),
    ("boundary-exactly-on-the-limit", [65536, 65536, 1]),
    ("limit-then-one", [CHUNK, 1]),
    ("one-cell-short-of-the-limit", [CHUNK - 1, 1, 1]),
    ("a-single-problem-larger-than-the-limit", [CHUNK + 1, 5]),
    ("a-larger-problem-in-the-middle", [5, 200000, 5]),
    ("a-larger-problem-last", [5, 5, BIG - 1]),
    ("skipped-problems", [0, 0, 3, 0]),
    ("only-skipped-problems", [0, 0, 0]),
    ("1024-of-128", [128] * 1024),
    ("1025-of-128", [128] * 1025),
    ("uneven", [(911 * i) % 40000 for i in range(60)]),
]
RUNS = [  # (name, problems as (source start, length, takes part))
    ("none", []),
    ("all-take-part", laid_out([3, 1, 5, 2])),
    ("skipped-first", laid_out([2, 3, 4], {0})),
    ("skipped-last", laid_out([2, 3, 4], {2})),
    ("skipped-only", laid_out([5], {0})),
    ("skipped-middle", laid_out([2, 3, 4], {1})),
    ("two-skipped-in-a-row", laid_out([1, 2, 3, 4, 5], {1, 2})),
    ("all-skipped", laid_out([1, 2, 3], {0, 1, 2})),
    ("empty-problems-take-part", laid_out([0, 3, 0, 0, 2, 0])),
    ("an-empty-problem-skipped-between-two", laid_out([3, 0, 2], {1})),  # it holds no entry: the source is continuous across it
    ("an-empty-problem-beside-a-skipped-one", laid_out([3, 0, 2, 5, 1], {1, 2})),
    ("skipped-first-and-last", laid_out([4, 1, 1, 4], {0, 3})),
    ("alternating", laid_out([1, 2, 3, 4, 5, 1], {0, 2, 4})),
    ("places-with-gaps", [(0, 4, 1), (8, 4, 1), (12, 4, 1), (20, 4, 1)]),  # the kept columns 0, 2, 3, 5 of four blobs
    ("places-out-of-order", [(8, 4, 1), (0, 4, 1), (4, 4, 1)]),
    ("beyond-the-bound-skipped", [(0, 5, 1), (5, BIG, 0), (5 + BIG, 2, 1)]),
]
KEEP = [  # (name, n_blobs, column indices)
    ("none-refused", 6, list(range(128))),
    ("all-refused", 6, [128, 129, 1 << 63, 500]),
    ("alternating", 6, [0, 128, 1, 999, 127, 128, 2]),
    ("first-and-last-refused", 3, [128, 5, 6, 128]),
    ("no-columns", 6, []),
    ("no-blobs-keeps-every-index", 0, [5, 500, 1 << 40]),
    ("too-many-blobs-refuses-every-index", BIG, [0, 5, 127]),
    ("largest-blob-count", BIG - 1, [127, 128]),
]


def _cases():
    lines, want = [], []
    for consts, cases in (((MIN_PROBLEMS, MIN_CELLS, MAX_PARTS), PARTS), ((1, 1, 3), LOW_THRESHOLDS), ((1, 1, 1), LOW_THRESHOLDS), ((1, 1, 2), LOW_THRESHOLDS)):
        for _, cells in cases:
            lines.append("parts %d %d %d %d " % (*consts, len(cells)) + " ".join(map(str, cells)))
            want.append("parts " + ",".join(map(str, parts_rule(cells, *consts))))
    for _, n in CHUNKS:
        lines.append("chunks %d %d " % (CHUNK, len(n)) + " ".join(map(str, n)))
        want.append("chunks " + ",".join(map(str, chunks_rule(n, CHUNK))))
    for _, problems in RUNS:
        lines.append("runs %d " % len(problems) + " ".join("%d %d %d" % p for p in problems))
        want.append("runs " + ",".join("%d:%d:%d" % r for r in runs_rule([p if p[1] < BIG else (p[0], 0, 0) for p in problems])))
    for _, nb, idx in KEEP:
        lines.append("keep %d %d " % (nb, len(idx)) + " ".join(map(str, idx)))
        want.append("keep " + ",".join(str(b) for b, i in enumerate(idx) if D.validation_status(nb, i) == 0))
    return lines, want


@pytest.fixture(scope="module", params=list(BUILDS))
def printed(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vm_plan_" + request.param)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, cases = str(tmp / "test_vm_plan"), str(tmp / "cases.txt")
    subprocess.check_call([hipcc, *BUILDS[request.param], "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_vm_plan.cpp"), "-o", exe])
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


def _numbers(row):
    tail = row.split(" ", 1)[1].strip() if " " in row else ""
    return [int(x) for x in tail.split(",")] if tail else []


def test_the_constants_are_the_engines():
    text = open(os.path.join(CSRC, "engine.hpp")).read()
    found = re.search(r"VM_SPLIT_MIN_PROBLEMS = (\d+), VM_SPLIT_MIN_CELLS = (\d+), VM_CHUNK_CELLS = (\d+);", text)
    assert found and tuple(map(int, found.groups())) == (MIN_PROBLEMS, MIN_CELLS, CHUNK)
    assert re.search(r"static constexpr int VM_SLOTS = 3;", text) and MAX_PARTS == 3  # (verify_many.hip: at most three parts, and a slot for each)


@pytest.mark.timeout(600)
def test_the_parts_of_a_call(printed):
    rows = _rows(printed, "parts", len(PARTS) + 3 * len(LOW_THRESHOLDS))
    for l, g, w in rows:
        assert g.strip() == w.strip(), l[:60]
        head = l.split()
        min_problems, min_cells, max_parts, B = map(int, head[1:5])
        cells, cuts = list(map(int, head[5:])), _numbers(g)
        assert cuts[0] == 0 and cuts[-1] == B and cuts == sorted(set(cuts)) and len(cuts) - 1 <= max_parts  # a partition into non-empty parts
        if B < min_problems or sum(cells) < min_cells:
            assert cuts == ([0, B] if B else [0])  # no cut below either threshold
    by_name = {name: _numbers(g) for (name, _), (l, g, w) in zip(PARTS, rows)}
    assert by_name["B=0"] == [0] and by_name["B=1"] == [0, 1] and by_name["B=191-many-cells"] == [0, 191]
    assert by_name["B=192-24575-cells"] == [0, 192] and by_name["B=193-24575-cells"] == [0, 193]
    assert by_name["B=192-24576-cells"] == [0, 64, 128, 192] and by_name["1024-of-128"] == [0, 342, 683, 1024]
    assert by_name["one-problem-above-two-thirds-first"] == [0, 1, 2, 200]  # one cut per problem: the second behind the next one
    assert by_name["one-problem-above-two-thirds-last"] == [0, 200] and by_name["everything-in-the-last-problem"] == [0, 200]
    assert by_name["three-equal-problems"] == [0, 3]
    low = {name: _numbers(g) for (name, _), (l, g, w) in zip(LOW_THRESHOLDS, rows[len(PARTS):])}
    assert low["three-equal-problems"] == [0, 1, 2, 3] and low["one-problem"] == [0, 1] and low["zeros"] == [0, 4]


@pytest.mark.timeout(600)
def test_the_chunks_of_a_part(printed):
    rows = _rows(printed, "chunks", len(CHUNKS))
    for (name, n), (l, g, w) in zip(CHUNKS, rows):
        assert g.strip() == w.strip(), name
        ends = _numbers(g)
        assert ends[0] == 0 and ends[-1] == len(n) and ends == sorted(set(ends)), name  # a partition into non-empty chunks
        for b0, b1 in zip(ends, ends[1:]):
            assert sum(n[b0:b1]) <= CHUNK or b1 == b0 + 1, name
            assert b1 == len(n) or sum(n[b0:b1 + 1]) > CHUNK, name  # and none ends early
    by_name = {name: _numbers(g) for (name, _), (l, g, w) in zip(CHUNKS, rows)}
    assert by_name["boundary-exactly-on-the-limit"] == [0, 2, 3] and by_name["limit-then-one"] == [0, 1, 2]
    assert by_name["a-single-problem-larger-than-the-limit"] == [0, 1, 2] and by_name["a-larger-problem-in-the-middle"] == [0, 1, 2, 3]
    assert by_name["1024-of-128"] == [0, 1024] and by_name["1025-of-128"] == [0, 1024, 1025] and by_name["none"] == [0]


@pytest.mark.timeout(600)
def test_the_copy_runs_of_a_problem_list(printed):
    rows = _rows(printed, "runs", len(RUNS))
    for (name, problems), (l, g, w) in zip(RUNS, rows):
        assert g.strip() == w.strip(), name
        tail = g.split(" ", 1)[1].strip()
        runs = [tuple(int(x) for x in r.split(":")) for r in tail.split(",")] if tail else []
        small = [p if p[1] < BIG else (p[0], 0, 0) for p in problems]  # (the problem beyond the bound is skipped: not expanded here)
        assert [src + j for src, length, _ in runs for j in range(length)] == entries(small), name  # exactly the participants, in order
        at = 0
        for src, length, dst in runs:
            assert length > 0 and dst == at, name  # destinations back to back
            at += length
        out = {p[0] + j for p in problems if not p[2] for j in range(min(p[1], 64))}  # entries of the problems that take no part
        assert not out & {src + j for src, length, _ in runs for j in range(length)}, name  # no run spans a skipped problem's entries
        for (s0, l0, _), (s1, _, _) in zip(runs, runs[1:]):
            assert s0 + l0 != s1, name  # and none ends where the source goes on
    by_name = {name: g.split(" ", 1)[1].strip() for (name, _), (l, g, w) in zip(RUNS, rows)}
    assert by_name["all-take-part"] == "0:11:0" and by_name["skipped-middle"] == "0:2:0,5:4:2" and by_name["skipped-only"] == ""
    assert by_name["two-skipped-in-a-row"] == "0:1:0,6:9:1" and by_name["an-empty-problem-skipped-between-two"] == "0:5:0"
    assert by_name["an-empty-problem-beside-a-skipped-one"] == "0:3:0,5:6:3" and by_name["places-with-gaps"] == "0:4:0,8:8:4,20:4:12"
    assert by_name["beyond-the-bound-skipped"] == "0:5:0,%d:2:5" % (5 + BIG)


@pytest.mark.timeout(600)
def test_the_kept_columns_are_those_validation_accepts(printed):
    for (name, nb, idx), (l, g, w) in zip(KEEP, _rows(printed, "keep", len(KEEP))):
        assert g.strip() == w.strip(), name
        assert _numbers(g) == [b for b, i in enumerate(idx) if D.validation_status(nb, i) == 0], name
    by_name = {name: _numbers(g) for (name, _, _), (l, g, w) in zip(KEEP, _rows(printed, "keep", len(KEEP)))}
    assert by_name["all-refused"] == [] and by_name["alternating"] == [0, 2, 4, 6] and by_name["none-refused"] == list(range(128))
    assert by_name["no-blobs-keeps-every-index"] == [0, 1, 2] and by_name["too-many-blobs-refuses-every-index"] == []
