"""The batch verifiers' Fiat-Shamir challenges and pairing inputs, byte for byte (tests/verify_transcript.py is the statement and the cases).

A verdict does not depend on the challenge: for valid inputs the batched equation holds for any weights, for a tampered input any
non-zero weight rejects.  A transcript that leaves out bytes, a wrong entry of the power table, a weight or interpolation kernel that
drops the same cells from all three sums all pass every `is True` / `is False` assertion.  The two G1 points handed to the pairing
check depend on all of it, and eth_kzg_amd_verify_cell_kzg_proof_batch_partial hands them out for any range of a batch.

Non-GPU leg: the Python statement against the oracle's export (the function its golden-vector verdicts come from) on every case, the
range partials of the statement against the whole, and the generator's own conditions.
GPU leg: the partial call in both forms of the lincombs (windowed MSM + k_interp; byte-shifted MSM + k_interp_cells / k_interp_sum), the
device-resident form through a hook that shares the product's set-up, the blob batch verifier in its host and device forms; every
verdict through the public entry points.

The many path (eth_kzg_amd_verify_cell_kzg_proof_batch_many, where concurrent single calls end up too) shares none of those kernels
behind the challenge.  eth_kzg_amd_test_verify_many_sums runs one pass of it with a tap on its pinned read-backs: every problem's pair,
the folding weights, the folded pair and every probe of the search for wrong problems are compared with the statement byte for byte,
in every form a pass takes (T.many_cases(): the pass-to-kernel map stands next to it), and the form the hook reports is asserted.
Non-GPU leg: the passes' conditions and five faults no verdict shows, made in the statement's scalars."""
import ctypes as C
import hashlib
import importlib
import json
import os
import subprocess
import sys
import time

import pytest

import verify_transcript as T
from many_coop_off_check import many_sums

kzg = importlib.import_module("rust-eth-kzg_amd")
CELL_CASES = {c.name: c for c in T.cell_cases()}
MANY_PASSES = {p.name: p for p in T.many_cases()}
COOP_POINTS_MAX = 8192  # launch::coop_points_max() (csrc/k_g1misc.hip) where ETH_KZG_AMD_COOP_POINTS is not set
BLOB_CASES = {c.name: c for c in T.blob_cases()}
_statement = {}  # (material fingerprint, case, lo, hi) -> bytes: computed once, shared by both legs, never changed


def _fingerprint(mat):
    h = hashlib.sha256()
    for b in range(len(mat.blobs)):
        h.update(mat.commitments[b] + mat.blob_proofs[b] + b"".join(mat.cells[b]) + b"".join(mat.proofs[b]))
    return h.digest()


def _challenge(mat, fp, case):
    key = (fp, case.name, "r")
    if key not in _statement:
        _statement[key] = T.cell_challenge(*case.args(mat))
    return _statement[key]


def _partial(mat, fp, case, lo, hi):
    key = (fp, case.name, lo, hi)
    if key not in _statement:
        _statement[key] = T.cell_partial(*case.args(mat), lo, hi, _challenge(mat, fp, case))
    return _statement[key]


def _blob_inputs(mat, fp, case):
    key = (fp, "blobs", case.name)
    if key not in _statement:
        _statement[key] = T.blob_batch_inputs(*case.args(mat))
    return _statement[key]


def _problem_sums(mat, fp, q):
    """the two pairing inputs of a live problem of a pass: the whole batch of its (possibly changed) arguments"""
    n = len(q.case.entries)
    if q.kind == "valid" and q.case.name in CELL_CASES:
        return _partial(mat, fp, q.case, 0, n)  # shared with the partial tests
    key = (fp, "many", q.name)
    if key not in _statement:
        _statement[key] = T.cell_partial(*q.args(mat), 0, n)
    return _statement[key]


def _pass_statement(mat, fp, p):
    """-> (sums[B] (None where the problem takes no part), rho[B], the folded pair or None)"""
    key = (fp, "pass", p.name)
    if key not in _statement:
        sums = [_problem_sums(mat, fp, q) if q.live else None for q in p.problems]
        digests = [T.cell_digest(*q.args(mat)) if q.hashed else bytes(32) for q in p.problems]
        rho = T.fold_weights(digests, [q.live for q in p.problems])
        _statement[key] = (sums, rho, T.fold_pair(sums, rho, 0, len(sums)) if p.folded else None)
    return _statement[key]


# ---- non-GPU leg -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_material(oracle):
    blobs = T.material_blobs()
    cp = [oracle.compute_cells_and_kzg_proofs(b) for b in blobs]
    comms = [oracle.blob_to_kzg_commitment(b) for b in blobs]
    mat = T.Material(blobs, comms, [c for c, _ in cp], [p for _, p in cp], [oracle.compute_blob_kzg_proof(b, c) for b, c in zip(blobs, comms)])
    return mat, _fingerprint(mat)


def test_the_cases_are_the_ones_asked_for():
    names = list(CELL_CASES)
    assert [CELL_CASES["len-%d" % n].expect["n"] for n in T.LENGTHS] == list(T.LENGTHS) == [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025]
    assert CELL_CASES["ranges-of-300"].ranges == [(0, 300), (0, 1), (299, 300), (5, 200), (255, 257)]
    assert CELL_CASES["exponents-to-2^13"].ranges == [(0, 8200), (8190, 8200), (4090, 4100)]
    assert [len(c.picks) for c in BLOB_CASES.values()] == [1, 2, 3, 17]
    assert [c.name for c in T.cell_cases()] == names and T.cell_cases()[0].entries == CELL_CASES[names[0]].entries  # a plain function of the seed
    assert T.cell_cases("another seed")[4].entries != CELL_CASES[names[4]].entries
    # entries 14 .. 23 of the power table need batches of 16385 cells and more
    assert T.table_entries_reached(CELL_CASES.values()) == list(range(14))


@pytest.mark.parametrize("name", list(CELL_CASES))
def test_cell_statement_matches_the_oracle_export(cpu_material, oracle, name):
    mat, fp = cpu_material
    case = CELL_CASES[name]
    case.check(mat)
    args = case.args(mat)
    n = len(args[1])
    r_be, out96, ok = oracle.verify_cell_kzg_proof_batch_inputs(*args)
    assert T.fr_be(_challenge(mat, fp, case)) == r_be, name
    whole = _partial(mat, fp, case, 0, n)
    assert whole == out96, name
    assert ok is True  # the verdict of the function the bytes come from: the ones compared are the ones paired (oracle/kzg.c)
    # the range partials add up to the whole: the batch cut at every bound of the case's ranges
    cuts = sorted({0, n} | {b for rg in case.ranges for b in rg})
    parts = [_partial(mat, fp, case, lo, hi) for lo, hi in zip(cuts, cuts[1:])]
    assert T.g1_sum([p[:48] for p in parts]) == whole[:48] and T.g1_sum([p[48:] for p in parts]) == whole[48:], name
    assert T.cell_partial(*args, 0, 0, 1) == T.INF + T.INF


@pytest.mark.parametrize("name", list(BLOB_CASES))
def test_blob_batch_statement_matches_the_oracle_export(cpu_material, oracle, name):
    mat, fp = cpu_material
    case = BLOB_CASES[name]
    case.check(mat)
    args = case.args(mat)
    r, out96 = _blob_inputs(mat, fp, case)
    r_be, want96, ok = oracle.verify_blob_kzg_proof_batch_inputs(*args)
    assert T.fr_be(r) == r_be and out96 == want96, name
    assert ok is True and oracle.verify_blob_kzg_proof_batch(*args) is True


def test_the_statement_sees_what_a_verdict_does_not(cpu_material, oracle):
    """the bytes move with every part of the transcript (so leaving a part out shows) while the verdict of a valid batch does not"""
    mat, fp = cpu_material
    case = CELL_CASES["four-interleaved"]
    comm, idx, cells, proofs = case.args(mat)
    base = _partial(mat, fp, case, 0, len(idx))
    # the same multiset of entries in another order: other row indices and exponents, still valid
    order = list(range(len(idx)))
    order[0], order[1] = order[1], order[0]
    swapped = [[col[i] for i in order] for col in (comm, idx, cells, proofs)]
    assert oracle.verify_cell_kzg_proof_batch(*swapped) is True
    r_be, out96, ok = oracle.verify_cell_kzg_proof_batch_inputs(*swapped)
    assert ok and out96 != base and T.cell_partial(*swapped, 0, len(idx)) == out96


def test_the_cases_separate_three_known_faults(cpu_material):
    """Three faults no verdict shows, made in the statement's own scalars: which (case, range) pairs move.  A power table whose entry 9
    repeats entry 8 moves every range with an exponent k >= 512; a transcript without the row index moves r everywhere; row weights
    summed over the first 256 cells of a range only move every range longer than 256 that has a row member behind them."""
    mat, fp = cpu_material
    moved = {"table-entry-9": set(), "no-row-index": set(), "weights-capped-256": set()}
    for case in CELL_CASES.values():
        comm, idx, cells, proofs = case.args(mat)
        uniq, row = T.dedup(comm)
        r = _challenge(mat, fp, case)
        h = hashlib.sha256(b"RCKZGCBATCH__V1_" + T.be64(4096) + T.be64(64) + T.be64(len(uniq)) + T.be64(len(idx)) + b"".join(uniq))
        for k in range(len(idx)):
            h.update(T.be64(idx[k]) + cells[k] + proofs[k])
        if T.reduce_digest(h.digest()) != r:
            moved["no-row-index"].add(case.name)
        tab = [pow(r, 1 << i, T.R) for i in range(24)]
        tab[9] = tab[8]
        for lo, hi in case.ranges:
            for k in range(lo, hi):
                bad = 1
                for i in range(24):
                    if k >> i & 1:
                        bad = bad * tab[i] % T.R
                if bad != pow(r, k, T.R):
                    moved["table-entry-9"].add((case.name, lo, hi))
                    break
            w = [0] * len(uniq)
            for k in range(lo + 256, hi):  # what a scan capped at 256 cells leaves out
                w[row[k]] = (w[row[k]] + pow(r, k, T.R)) % T.R
            if any(w):
                moved["weights-capped-256"].add((case.name, lo, hi))
    assert moved["no-row-index"] == set(CELL_CASES)
    assert moved["table-entry-9"] == {("len-1023", 0, 1023), ("len-1025", 0, 1025), ("exponents-to-2^13", 0, 8200),
                                      ("exponents-to-2^13", 8190, 8200), ("exponents-to-2^13", 4090, 4100)}
    assert {c for c, _, _ in moved["weights-capped-256"]} == {"len-257", "len-1023", "len-1025", "row-of-280-next-to-row-of-1", "ranges-of-300",
                                                              "exponents-to-2^13"}


def test_the_many_passes_are_the_ones_asked_for():
    assert list(MANY_PASSES) == ["short-four-lanes", "short-holes", "short-one-lane", "large-folded", "large-one-live", "search", "folded-ten"]
    for p in MANY_PASSES.values():
        p.check(T.MANY_HOST_THREADS, COOP_POINTS_MAX)
    assert [q.name for q in T.many_cases()[5].problems] == [q.name for q in MANY_PASSES["search"].problems]  # a plain function of the seed
    assert [q.case.entries for q in T.many_cases("another seed")[5].problems] != [q.case.entries for q in MANY_PASSES["search"].problems]
    assert [q.name for q in MANY_PASSES["short-four-lanes"].problems] == ["len-1", "len-65", "four-interleaved", "identity-commitment-mixed"]
    assert sorted(q.name for q in MANY_PASSES["large-folded"].problems) == sorted(
        ["len-1", "len-2", "len-63", "len-64", "len-65", "len-255", "len-256", "len-257", "one-commitment", "row-of-280-next-to-row-of-1",
         "identity-commitment-only", "constant-polynomial", "cells-of-r-minus-1", "one-index", "all-128-indices"])
    # the one-lane short-chain pass by size: 3 n + 2 m + 64 B products and subgroup tests against 2 * coop_points_max()
    n, m = MANY_PASSES["short-one-lane"].cells()
    assert (n, m) == (8200, 3) and 3 * n + 2 * m + 64 * 1 > 2 * COOP_POINTS_MAX
    # the search: one pass, the wrong problems where they were asked for, a skipped and a refused problem in between, 1 .. 3 cells each
    s = MANY_PASSES["search"]
    assert len(s.problems) == 300 and s.cells()[0] < 24576
    assert [i for i, q in enumerate(s.problems) if q.kind == "swapped"] == [0, 150, 299]
    assert s.problems[40].kind == "empty" and s.problems[200].kind == "off-subgroup" and s.problems[200].status == 2
    assert {len(q.case.entries) for q in s.problems if q.kind != "empty"} == {1, 2, 3}
    # the search under two helper threads: two-way splits, per-problem checks from 2 T suspects; a probe wider than the 128 lanes of
    # k_vm_fold_ranges, and widths between 2 and 127 that are no powers of two (the folds it skips: span >= width)
    plan = T.search_plan([q.live for q in s.problems], [q.verdict for q in s.problems], T.MANY_HOST_THREADS)
    widths = [hi - lo for lo, hi, _ in plan]
    assert widths[:2] == [150, 150] and max(widths) > 128
    assert len({w for w in widths if 2 <= w <= 127 and w & (w - 1)}) >= 5, widths
    assert [(lo, hi) for lo, hi, ok in plan if hi - lo == 1 and not ok] == [(0, 1), (150, 151)]  # exact by their own weighted pair
    assert plan[-1][:2] == (298, 300)  # two suspects are left to the per-problem checks


def _many_scalars(mat, p, fault=None):
    """What the many-verification multiplies points by, in exact integers: per live problem the powers r_b^k and the row weights (the
    proof scalars, the coset factors and the interpolation sums are these powers times constants), per folded pass the weights of the
    folded pair and of every probe.  fault: one of the five wrong kernels below, made in these scalars."""
    args = [q.args(mat) for q in p.problems]
    held = [q.kind not in ("empty", "bad-index") for q in p.problems]  # problems whose cells lie in the pass's arrays
    rs = [T.reduce_digest(T.cell_digest(*a)) if h else None for a, h in zip(args, held)]
    start, pos = [], 0
    for a, h in zip(args, held):
        start.append(pos)
        pos += len(a[1]) if h else 0
    out, powers = {}, {}
    for b, q in enumerate(p.problems):
        if not held[b]:
            continue
        r = rs[0] if fault == "table-of-problem-0" else rs[b]
        powers[b] = [pow(r, (start[b] if fault == "position-in-pass" else 0) + k, T.R) for k in range(len(args[b][1]))]
    for b, q in enumerate(p.problems):
        if not q.live:
            continue
        uniq, row = T.dedup(args[b][0])
        w = [0] * len(uniq)
        for k, i in enumerate(row):
            w[i] = (w[i] + powers[b][k]) % T.R
        if fault == "weights-across-problems":  # every cell of the pass that carries the row's commitment bytes
            for o in range(len(p.problems)):
                if o != b and held[o]:
                    for k, c in enumerate(args[o][0]):
                        if c in uniq:
                            w[uniq.index(c)] = (w[uniq.index(c)] + powers[o][k]) % T.R
        out[("problem", b)] = (tuple(powers[b]), tuple(w))
    if p.folded:
        live = [q.live for q in p.problems]
        digests = [T.cell_digest(*a) if q.hashed else bytes(32) for a, q in zip(args, p.problems)]
        rho = T.fold_weights(digests, live)
        if fault == "fold-index-among-live":
            dense = T.fold_weights(digests, [True] * len(live))
            rho, i = [], 0
            for on in live:
                rho.append(dense[i] if on else 0)
                i += on
        if fault == "rho-low-word":
            rho = [v & 0xffffffff for v in rho]
        out[("fold",)] = tuple(rho)
        if p.searched:
            for lo, hi, _ in T.search_plan(live, [q.verdict for q in p.problems], T.MANY_HOST_THREADS):
                out[("probe", lo, hi)] = tuple(rho[lo:hi])
    return out


def test_the_many_cases_separate_known_faults(cpu_material):
    """Five faults no verdict shows, made in the statement's own scalars: which (pass, problem) pairs, folded pairs and probes move."""
    mat, _ = cpu_material
    moved = {}
    for fault in ("table-of-problem-0", "position-in-pass", "rho-low-word", "fold-index-among-live", "weights-across-problems"):
        moved[fault] = set()
        for p in MANY_PASSES.values():
            good, bad = _many_scalars(mat, p), _many_scalars(mat, p, fault)
            assert good.keys() == bad.keys()
            moved[fault] |= {(p.name,) + k for k in good if good[k] != bad[k]}
    live = {(p.name, "problem", b): q for p in MANY_PASSES.values() for b, q in enumerate(p.problems) if q.live}
    folds = {(p.name, "fold") for p in MANY_PASSES.values() if p.folded}
    probes = {k for f in moved.values() for k in f if k[1] == "probe"}
    # (a) every problem behind the first with two cells or more; a problem of ONE cell uses r^0 only and must not move
    assert moved["table-of-problem-0"] == {k for k, q in live.items() if k[2] >= 1 and len(q.case.entries) >= 2}
    one_cell = {k for k, q in live.items() if k[2] >= 1 and len(q.case.entries) == 1}
    assert len(one_cell) > 50 and not one_cell & moved["table-of-problem-0"], "a one-cell problem uses only r^0: problem 0's table gives the same"
    # (b) every problem behind the first (problem 0 of every pass holds cells: ManyPass.check)
    assert moved["position-in-pass"] == {k for k in live if k[2] >= 1}
    # (c) the folded pairs and the probes, and nothing else
    plan = {("search", "probe", lo, hi) for lo, hi, _ in T.search_plan(*[[getattr(q, a) for q in MANY_PASSES["search"].problems] for a in ("live", "verdict")],
                                                                      T.MANY_HOST_THREADS)}
    assert moved["rho-low-word"] == folds | plan and len(plan) == 42 and probes == plan
    # (d) only passes with a hole in front of a live problem, there the folded pair and the probes that hold a problem behind the hole
    assert {k[0] for k in moved["fold-index-among-live"]} == {"search", "folded-ten"} == {p.name for p in MANY_PASSES.values()
                                                                                        if p.folded and p.expect["hole_before_live"]}
    assert moved["fold-index-among-live"] == {("search", "fold"), ("folded-ten", "fold")} | {k for k in plan if k[3] > T.SEARCH_EMPTY + 1}
    # (e) only problems that share a commitment with another problem of their pass; in the two long passes that is a NEIGHBOUR (a kernel
    # that reads one problem too far is enough): ManyPass.check asserts there that what is shared is shared next door
    want = set()
    for p in MANY_PASSES.values():
        B = len(p.problems)
        want |= {(p.name, "problem", b) for b, q in enumerate(p.problems) if q.live and any(p.shares(b, o) for o in range(B))}
        if p.expect.get("sharing_is_adjacent"):
            assert all(p.shares(b, b - 1) or p.shares(b, b + 1) for n, _, b in want if n == p.name), p.name
    assert moved["weights-across-problems"] == want
    assert ("large-folded", "problem", 14) not in want and ("large-folded", "problem", 0) in want and len(want) > 300


def test_the_hooks_reject_missing_buffers():
    lib = kzg.load_library()
    if not hasattr(lib, "eth_kzg_amd_test_verify_cells_partial_device"):
        pytest.fail("the test hooks library (libc_eth_kzg_hooks.so) is not the library loaded")
    out, v = C.create_string_buffer(96), C.c_int32(0)
    assert lib.eth_kzg_amd_test_verify_cells_partial_device(None, 1, None, None, None, None, 0, 1, out) == 3
    assert lib.eth_kzg_amd_test_verify_blob_batch_inputs(None, 1, 0, None, None, None, out, C.byref(v)) == 3
    one = (C.c_uint64 * 1)(1)
    args = [one, one, one, one, one, one, one, one, (C.c_int32 * 1)(), (C.c_int32 * 1)(), (C.c_int32 * 4)(), out, (C.c_uint32 * 4)(), out,
            (C.c_int32 * 3)(), out, 1, one]
    for missing in range(len(args)):
        if missing != 16:  # (the count of probe buffers)
            assert lib.eth_kzg_amd_test_verify_many_sums(None, 1, *[None if i == missing else a for i, a in enumerate(args)]) == 3, missing


# ---- GPU leg -------------------------------------------------------------------------------------------------------------------------------
def _ctx(**env):
    import torch
    torch.cuda.init()
    env = dict(env, ETH_KZG_AMD_TABLE_GB="3")  # the start tables: results never depend on the table
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
def forms():
    """{"windowed": msm_pippenger2 + k_interp, "shifted": shifted point copies + k_interp_cells / k_interp_sum} at every batch size"""
    c = {"windowed": _ctx(ETH_KZG_AMD_PIP_SHIFT_MIN=str(1 << 20)), "shifted": _ctx(ETH_KZG_AMD_PIP_SHIFT_MIN="1")}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def gpu_material(forms, oracle):
    ctx = forms["windowed"]
    blobs = T.material_blobs()
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(blobs)
    assert st == [0] * len(blobs)
    assert (cells[0], proofs[0]) == tuple(oracle.compute_cells_and_kzg_proofs(blobs[0]))
    comms = [ctx.blob_to_kzg_commitment(b) for b in blobs]
    st, bp = ctx.compute_blob_kzg_proof_batch(blobs, comms)
    assert st == [0] * len(blobs) and comms[0] == oracle.blob_to_kzg_commitment(blobs[0]) and bp[0] == oracle.compute_blob_kzg_proof(blobs[0], comms[0])
    mat = T.Material(blobs, comms, cells, proofs, bp)
    return mat, _fingerprint(mat)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CELL_CASES))
def test_cell_partials_equal_the_statement_in_both_forms(forms, gpu_material, name):
    mat, fp = gpu_material
    case = CELL_CASES[name]
    case.check(mat)
    args = case.args(mat)
    bad = []
    for form, ctx in forms.items():
        for lo, hi in case.ranges:
            got, want = ctx.verify_cell_kzg_proof_batch_partial(*args, lo, hi), _partial(mat, fp, case, lo, hi)
            if got != want:
                bad.append((form, lo, hi, got[:48] == want[:48], got[48:] == want[48:]))
        assert ctx.verify_cell_kzg_proof_batch(*args) is True, (name, form)
    assert not bad, "%s: (form, lo, hi, A equal, B equal) %s" % (name, bad)


DEVICE_RANGES = {"ranges-of-300": None, "len-1025": [(0, 1025), (100, 900), (1024, 1025)]}  # one chunk of the mirror; eight chunks


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DEVICE_RANGES))
def test_device_resident_partials_equal_the_statement(forms, gpu_material, name):
    import numpy as np
    import torch
    mat, fp = gpu_material
    case = CELL_CASES[name]
    comm, idx, cells, proofs = case.args(mat)
    n = len(idx)
    assert (n >= 512) == (name == "len-1025")  # verify.hip: eight chunks from 64 * VD_CHUNKS cells
    dev = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()  # noqa: E731
    d_c, d_l, d_p = dev(b"".join(comm)), dev(b"".join(cells)), dev(b"".join(proofs))
    d_i = torch.from_numpy(np.array(idx, dtype=np.int64)).cuda()
    torch.cuda.synchronize()
    lib = kzg.load_library()
    bad = []
    for form, ctx in forms.items():
        for lo, hi in DEVICE_RANGES[name] or case.ranges:
            out = C.create_string_buffer(96)
            rc = lib.eth_kzg_amd_test_verify_cells_partial_device(ctx.handle, n, d_c.data_ptr(), d_i.data_ptr(), d_l.data_ptr(), d_p.data_ptr(), lo, hi, out)
            assert rc == 0, (name, form, lo, hi, rc)
            want = _partial(mat, fp, case, lo, hi)
            if out.raw != want:
                bad.append((form, lo, hi))
        assert ctx.verify_cell_kzg_proof_batch_device(n, d_c.data_ptr(), d_i.data_ptr(), d_l.data_ptr(), d_p.data_ptr()) is True
    assert not bad, (name, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BLOB_CASES))
def test_blob_batch_sums_equal_the_statement_and_the_oracle(forms, gpu_material, oracle, name):
    import torch
    mat, fp = gpu_material
    case = BLOB_CASES[name]
    case.check(mat)
    blobs, comms, proofs = case.args(mat)
    n = len(blobs)
    r, want = _blob_inputs(mat, fp, case)
    r_be, oracle96, ok = oracle.verify_blob_kzg_proof_batch_inputs(blobs, comms, proofs)
    assert ok and oracle96 == want and r_be == T.fr_be(r)
    ctx = forms["windowed"]
    lib = kzg.load_library()
    ba, _k1 = kzg._ptr_array(blobs)
    ca, _k2 = kzg._ptr_array(comms)
    pa, _k3 = kzg._ptr_array(proofs)
    out, v = C.create_string_buffer(96), C.c_int32(0)
    assert lib.eth_kzg_amd_test_verify_blob_batch_inputs(ctx.handle, n, 0, ba, ca, pa, out, C.byref(v)) == 0
    assert out.raw == want and v.value == 1, (name, "host form")
    dev = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()  # noqa: E731
    d_b, d_c, d_p = dev(b"".join(blobs)), dev(b"".join(comms)), dev(b"".join(proofs))
    torch.cuda.synchronize()
    out, v = C.create_string_buffer(96), C.c_int32(0)
    assert lib.eth_kzg_amd_test_verify_blob_batch_inputs(ctx.handle, n, 1, d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), out, C.byref(v)) == 0
    assert out.raw == want and v.value == 1, (name, "device form")
    assert ctx.verify_blob_kzg_proof_batch(blobs, comms, proofs) is True
    assert ctx.verify_blob_kzg_proof_batch_device(n, d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr()) is True


# ---- the many-verification: one pass through eth_kzg_amd_test_verify_many_sums ------------------------------------------------------------
@pytest.fixture(scope="module")
def many_ctx():
    """two helper threads: a pass of <= 4 problems is short-chain, the search splits two ways and hands <= 4 suspects to per-problem checks"""
    c = _ctx(ETH_KZG_AMD_HOST_THREADS=str(T.MANY_HOST_THREADS))
    yield c
    c.close()


def _probe_statement(fp, p, sums, rho, lo, hi):
    key = (fp, "probe", p.name, lo, hi)
    if key not in _statement:
        _statement[key] = T.fold_pair(sums, rho, lo, hi)
    return _statement[key]


IN_PROCESS = [name for name in MANY_PASSES if name != "folded-ten"]  # (that one runs with the four-lane kernels switched off, below)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IN_PROCESS)
def test_many_pass_sums_fold_and_probes_equal_the_statement(many_ctx, gpu_material, name):
    mat, fp = gpu_material
    p = MANY_PASSES[name]
    p.check(T.MANY_HOST_THREADS, COOP_POINTS_MAX)
    problems = [q.args(mat) for q in p.problems]
    sums, rho, fold = _pass_statement(mat, fp, p)
    live, verdicts = [q.live for q in p.problems], [q.verdict for q in p.problems]
    t0 = time.perf_counter()
    rc, got = many_sums(many_ctx, problems)
    print("%s: hook %.3f s" % (name, time.perf_counter() - t0))
    assert rc == 0, (name, rc)
    # the form, from the engine's own expressions: a changed threshold must not quietly move the pass to other kernels
    small = len(problems) <= 2 * T.MANY_HOST_THREADS
    folded = not small and sum(live) >= 2
    assert (got.small, got.folded) == (small, folded) == (p.small, p.folded), (name, got.small, got.folded)
    assert got.searched == p.searched, name
    assert got.status == [q.status for q in p.problems], (name, got.status)
    assert got.verified == verdicts, (name, [b for b in range(len(verdicts)) if got.verified[b] != verdicts[b]])
    bad = [(b, got.sums[b][:48] == sums[b][:48], got.sums[b][48:] == sums[b][48:]) for b in range(len(problems)) if live[b] and got.sums[b] != sums[b]]
    assert not bad, "%s: (problem, A equal, B equal) %s" % (name, bad[:20])
    if folded:
        assert got.rho == rho, (name, [b for b in range(len(rho)) if got.rho[b] != rho[b]][:20])
        assert got.fold == fold, (name, got.fold[:48] == fold[:48], got.fold[48:] == fold[48:])
        assert got.fold_verdict == (1 if all(v for v, on in zip(verdicts, live) if on) else 0), name
    if p.searched:
        plan = T.search_plan(live, verdicts, T.MANY_HOST_THREADS)
        assert got.n_probes == len(got.probes) == len(plan), (name, got.n_probes)
        assert [(lo, hi, ok) for lo, hi, _, ok in got.probes] == plan, name  # the ranges in order, each flag = the exact verdicts it covers
        bad = [(lo, hi) for lo, hi, raw, _ in got.probes if raw != _probe_statement(fp, p, sums, rho, lo, hi)]
        assert not bad, (name, bad)
        widths = [hi - lo for lo, hi, _, _ in got.probes]
        assert max(widths) > 128 and len({w for w in widths if 2 <= w <= 127 and w & (w - 1)}) >= 5, widths
    else:
        assert got.n_probes == 0
    assert many_ctx.verify_cell_kzg_proof_batch_many(problems) == (got.verified, got.status), name


@pytest.mark.gpu
def test_the_hook_serves_one_pass_only(many_ctx, gpu_material):
    """a call the engine would cut into parts (192 problems with 24576 cells) is refused before anything is launched"""
    mat, _ = gpu_material
    one = CELL_CASES["all-128-indices"].args(mat)
    rc, _ = many_sums(many_ctx, [one] * 192)
    assert rc == 3
    rc, got = many_sums(many_ctx, [one] * 5)
    assert rc == 0 and got.folded and got.fold_verdict == 1 and got.verified == [True] * 5


@pytest.mark.gpu
def test_many_passes_with_the_four_lane_kernels_switched_off(many_ctx, gpu_material):
    """ETH_KZG_AMD_COOP_POINTS is read once per process: a child process runs the first short-chain pass (k_vm_products<VmLane>, the one-lane
    subgroup blocks) and a folded pass of ten problems (k_vm_fold_mul<VmLane>) and compares the same bytes (tests/many_coop_off_check.py).
    The same for the column source: a short-chain pass of 3 columns x 2 blobs and a folded one of 6 columns x 2 blobs whose blobs are one
    blob twice (n_u = 1 < n_blobs), through the column tap hook, against this process's bytes with the four-lane kernels on."""
    import data_columns as D
    from test_gpu_data_columns import column_sums
    mat, fp = gpu_material
    want = {"seed": T.SEED, "passes": {}}
    for name in ("short-four-lanes", "folded-ten"):
        p = MANY_PASSES[name]
        p.check(T.MANY_HOST_THREADS, COOP_POINTS_MAX)
        sums, _, fold = _pass_statement(mat, fp, p)
        want["passes"][name] = {"sums": [s.hex() if s else None for s in sums], "fold": fold.hex() if fold else None}
    want["columns"] = {}
    for name, picks, indices, form in (("3x2-short-chain", [0, 1], [127, 64, 1], [True, False]),
                                       ("6x2-folded-one-blob-twice", [0, 0], [127, 64, 1, 0, 5, 3], [False, True])):
        rc, got = column_sums(many_ctx, D.block(mat.commitments, mat.cells, mat.proofs, picks, indices), "host", 0)
        assert rc == 0 and [got.small, got.folded] == form and got.status == [0] * len(indices) and got.verified == [True] * len(indices), (name, rc)
        want["columns"][name] = {"picks": picks, "indices": indices, "form": form, "status": got.status, "verified": got.verified,
                                 "sums": [s.hex() for s in got.sums], "fold": got.fold.hex()}
    env = dict(os.environ, ETH_KZG_AMD_COOP_POINTS="0", ETH_KZG_AMD_HOST_THREADS=str(T.MANY_HOST_THREADS), ETH_KZG_AMD_TABLE_GB="3")
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "many_coop_off_check.py")], env=env,
                       input=json.dumps(want), capture_output=True, text=True, timeout=600)
    print("child process %.3f s" % (time.perf_counter() - t0))
    assert r.returncode == 0 and "many coop-off ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
