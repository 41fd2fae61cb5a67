"""The prover's G1 stage on the CPU (no GPU): the interpreter of tests/linmap_model.py runs the six compiled programs of the FK20
proofs map -- as tests/c/dump_linmap.cpp writes them out of the header the engine compiles them with -- over integers mod r and
must give the map's definition; and the plan of degenerate lanes that tests/test_gpu_g1_stage.py sends through the kernels is
solved here and its coverage COMPUTED from the operand values the interpreter records: every flag signature of every program
meets a = O, b = O, a = b, a = -b and a = b = O in some planned lane (a doubling run: operand = O), the constant multiplications
meet an identity operand in their first, a middle and their last launch, and a lane with such an operand sits next to a lane
without.  Run with -s for the table of signatures x classes per program."""
import random

import pytest

import linmap_model as M

R = M.R


@pytest.fixture(scope="module")
def plans():
    pool = M.pool_scalars()
    return {p.id: (p, M.plan_lanes(p, pool), M.generic_lanes(p, pool)) for p in M.programs()}


def test_the_dump_counts_the_programs_as_the_engine_builds_them():
    """operations per program: constant multiplications, additions and subtractions, doubling runs, fused pairs, launches, slots,
    distinct flag signatures (87 over the six programs, 32 distinct).  A compiler change that moves these numbers moves the plan of
    degenerate lanes with it: the coverage test below then says whether it still reaches everything."""
    want = {0: (298, 2378, 132, 452, 20, 852, 28), 1: (298, 2830, 132, 0, 20, 852, 28), 2: (712, 2420, 0, 0, 14, 1680, 2),
            3: (456, 3156, 128, 0, 19, 1168, 7), 4: (606, 2354, 16, 0, 16, 1468, 6), 5: (372, 3096, 132, 0, 20, 1000, 16)}
    all_sigs = set()
    for p in M.programs():
        idx = range(len(p.ops))
        mulc = sum(p.is_mulc(i) for i in idx)
        runs = sum(not p.is_mulc(i) and bool(p.ops[i][3] & 2) for i in idx)
        fused = sum(not p.is_mulc(i) and not p.ops[i][3] & 2 and bool(p.ops[i][3] & 4) for i in idx)
        assert (mulc, len(p.ops) - mulc - runs, runs, fused, len(p.launches), p.n_slots, len(p.signatures())) == want[p.id], p.id
        assert len(p.consts) == mulc
        all_sigs |= set(p.signatures())
    assert len(all_sigs) == 32


def test_the_interpreter_gives_the_definition_of_the_map():
    rng = random.Random(11)
    vectors = [[rng.randrange(R) for _ in range(128)] for _ in range(3)]
    vectors += [[0] * 128, [R - 1] * 128, [int(j == 5) for j in range(128)], [int(j % 2) * 7 for j in range(128)]]
    want = [M.proofs_of_linmap_inputs(x) for x in vectors]
    for p in M.programs():
        for x, w in zip(vectors, want):
            assert M.run(p, x) == w, p.id
    # the circulant form's scaling: u = y / 128 against x = y / 2
    y = vectors[0]
    assert M.proofs_of_circulant_inputs([v * pow(128, -1, R) % R for v in y]) == M.proofs_of_linmap_inputs([v * pow(2, -1, R) % R for v in y])


def test_every_result_of_every_operation_is_read_or_is_a_proof():
    """so that a wrong result of any operation -- either slot of a fused a + b / a - b pair -- has a way into the bytes compared"""
    for p in M.programs():
        pending = {}  # slot -> the operation whose result nobody has read yet
        for kind, first, count in p.launches:
            ops = range(first, first + count)
            for i in ops:
                dst, a, b, fl = p.ops[i]
                pending.pop(a, None)
                if kind != M.KIND_MULC and not fl & 2:
                    pending.pop(b, None)
            for i in ops:
                dst, a, b, fl = p.ops[i]
                for slot in [dst] + ([fl >> 16] if kind != M.KIND_MULC and not fl & 2 and fl & 4 else []):
                    assert slot not in pending, (p.id, i, "overwrites an unread result")
                    pending[slot] = i
        assert all(128 <= s < 256 for s in pending), (p.id, sorted(pending.items())[:4])
        assert sorted(pending) == list(range(128, 256))


def test_the_planned_lanes_reach_every_class_of_every_signature(plans):
    total = 0
    for pid, (p, lanes, generic) in sorted(plans.items()):
        needs = M.needs_of(p)
        hit_by = {nd: [] for nd in needs}
        for k, x in enumerate(lanes):
            assert M.run(p, x) == M.proofs_of_linmap_inputs(x)
            for h in M.hits_of(p, x):
                if h in hit_by:
                    hit_by[h].append(k)
        sigs = p.signatures()
        print(f"\nprogram {pid}: {len(lanes)} degenerate lanes, {len(sigs)} signatures, {len(needs)} signature x class pairs planned")
        print("  flags  run  " + "  ".join(f"{c:>7}" for c in M.CLASSES) + "   (lanes that reach the class)")
        for sig in sigs:
            row = [len(hit_by[(sig, c)]) if (sig, c) in hit_by else None for c in M.CLASSES]
            print(f"  0x{sig[0]:04x} {sig[1]:4d}  " + "  ".join(f"{'-' if v is None else v:>7}" for v in row))
        for li in sorted({nd[1] for nd in needs if nd[0] == "mulc"}):
            print(f"  constant multiplications, launch {li}: identity operand in lanes {hit_by[('mulc', li)]}")
        missing = [nd for nd in needs if not hit_by[nd]]
        print(f"  missing: {missing if missing else 'none'}")
        assert not missing, (pid, missing)
        assert len(generic) == 4
        for x in generic:
            assert not M.hits_of(p, x) and M.run(p, x) == M.proofs_of_linmap_inputs(x)
        total += len(lanes)
    print(f"\n{total} degenerate lanes over the six programs")
    assert total <= 64


@pytest.mark.parametrize("n", [12, 40, 70])
def test_the_batches_keep_the_coverage_and_put_the_lanes_at_the_edges(plans, n):
    """what tests/test_gpu_g1_stage.py runs at n lanes: all its batches together reach every need of the program (n = 12 needs
    more than one batch for the larger plans), a degenerate lane sits at each edge position, generic and all-identity lanes lie
    beside them, and some constant multiplication has an identity operand in one lane and a regular one in the lane next to it"""
    for pid, (p, lanes, generic) in sorted(plans.items()):
        batches = M.layout(n, len(lanes))
        assert len(batches) <= 2 and all(len(b) == n for b in batches)
        placed = {e[1] for b in batches for e in b if e[0] == "d"}
        assert placed == set(range(len(lanes)))
        reached = set()
        for k in placed:
            reached |= M.hits_of(p, lanes[k])
        assert not set(M.needs_of(p)) - reached
        neighbour = False
        for b in batches:
            for pos in M.edge_positions(n):
                assert b[pos][0] == "d", (pid, n, pos)
            assert b[1][0] == "g" and b[n - 2][0] == "g" and any(e[0] == "o" for e in b)
            recs = []
            for e in b:
                rec = []
                M.run(p, M.lane_inputs(e, lanes, generic), record=rec)
                recs.append(rec)
            for i in range(len(p.ops)):
                if p.is_mulc(i):
                    col = [r[i][0] for r in recs]
                    neighbour |= any((col[l] == 0) != (col[l + 1] == 0) and b[l][0] != "o" and b[l + 1][0] != "o" for l in range(n - 1))
        assert neighbour, (pid, n)
