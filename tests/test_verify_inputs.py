"""The batch verifiers' Fiat-Shamir challenges and pairing inputs, byte for byte (tests/verify_transcript.py is the statement and the cases).

A verdict does not depend on the challenge: for valid inputs the batched equation holds for any weights, for a tampered input any
non-zero weight rejects.  A transcript that leaves out bytes, a wrong entry of the power table, a weight or interpolation kernel that
drops the same cells from all three sums all pass every `is True` / `is False` assertion.  The two G1 points handed to the pairing
check depend on all of it, and eth_kzg_amd_verify_cell_kzg_proof_batch_partial hands them out for any range of a batch.

Non-GPU leg: the Python statement against the oracle's export (the function its golden-vector verdicts come from) on every case, the
range partials of the statement against the whole, and the generator's own conditions.
GPU leg: the partial call in both forms of the lincombs (windowed MSM + k_interp; byte-shifted MSM + k_interp_cells / k_interp_sum), the
device-resident form through a hook that shares the product's set-up, the blob batch verifier in its host and device forms; every
verdict through the public entry points."""
import ctypes as C
import hashlib
import importlib
import os

import pytest

import verify_transcript as T

kzg = importlib.import_module("rust-eth-kzg_amd")
CELL_CASES = {c.name: c for c in T.cell_cases()}
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


def test_the_hooks_reject_missing_buffers():
    lib = kzg.load_library()
    if not hasattr(lib, "eth_kzg_amd_test_verify_cells_partial_device"):
        pytest.fail("the test hooks library (libc_eth_kzg_hooks.so) is not the library loaded")
    out, v = C.create_string_buffer(96), C.c_int32(0)
    assert lib.eth_kzg_amd_test_verify_cells_partial_device(None, 1, None, None, None, None, 0, 1, out) == 3
    assert lib.eth_kzg_amd_test_verify_blob_batch_inputs(None, 1, 0, None, None, None, out, C.byref(v)) == 3


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
