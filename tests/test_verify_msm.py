"""The verifier's two-job bucket MSM (csrc/k_verify.hip) on its own, against exact integers, on inputs that the hash-made scalars and
seeded proofs of a verification never give it (tests/verify_msm_cases.py; the hook is eth_kzg_amd_test_verify_msm).

Non-GPU leg: the case generator reaches what each case is for -- checked on the item lists the kernels would build -- and the reference
(the affine group law of device_ops.py) agrees with the oracle's MSM and with the sums' discrete logarithms on every case.
GPU leg: every case through the windowed form, the byte-shifted form and the byte-shifted form as a verification launches it (four lanes
per point, and one lane per point in a process with the quad kernels switched off): byte equality of compressed points, nothing else.
Then the same shapes through the C ABI: one cell repeated 200 times, the zero blob's identity proofs 256 times."""
import collections
import importlib
import json
import os
import subprocess
import sys

import pytest

import device_ops as D
import synth
import verify_msm_cases as V

kzg = importlib.import_module("rust-eth-kzg_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = V.case_names()


def _lib():
    lib = kzg.load_library()
    if not hasattr(lib, "eth_kzg_amd_test_verify_msm"):
        pytest.fail("the test hooks library (libc_eth_kzg_hooks.so) is not the library loaded")
    return lib


# ---- non-GPU leg: the generator ------------------------------------------------------------------------------------------------------
def test_structured_scalars_split_as_built():
    for k, (k1, k2) in ((V.S01, (V.rep(1), V.rep(1))), (V.S80, (V.rep(0x80), V.rep(0x80))), (V.SAB, (V.rep(0xAB), V.rep(0xAB))),
                        (V.SFF, (V.rep(0xFF, 15), V.rep(0xFF, 15)))):
        assert V.split(k) == (k1, k2) and k < V.R and k1 < V.LAMBDA and k1 + k2 * V.LAMBDA == k
    assert V.rep(0xAC) > V.LAMBDA > V.rep(0xAB)  # no larger byte fills a half
    assert [V.split(k) for k in (V.LAMBDA - 1, V.LAMBDA, V.LAMBDA + 1, 2 * V.LAMBDA, V.R - 1)] == \
        [(V.LAMBDA - 1, 0), (0, 1), (1, 1), (0, 2), (0, V.LAMBDA + 1)]  # r - 1 = lambda (lambda + 1): the largest k2 there is
    for name in NAMES:  # a multiple of lambda has k1 = 0 somewhere; every count of the list is used
        if name.startswith("edge-scalars"):
            assert any(V.split(k)[0] == 0 and k for k in V.case(name).sc[1])
    assert {c.n for c in V.all_cases()} == set(V.COUNTS)
    assert V.cases(1)[0].sc == V.cases(1)[0].sc and V.cases(1)[0].sc != V.cases(2)[0].sc  # a plain function of the seed


def _copies(items):
    """-> the largest number of items of one bucket that are the same affine point, and from how many inputs they come"""
    by = collections.defaultdict(list)
    for it in items:
        if it[-1] is not None:
            by[it[-1]].append(it[0])
    best = max(by.values(), key=len, default=[])
    return len(best), max((len(set(v)) for v in by.values()), default=0)


def test_cases_reach_what_they_are_for():
    c = V.case("one-point-halves-01-64-129")
    for name in ("one-point-halves-01-64-129", "one-point-halves-80-129-200", "one-point-halves-ab-64-129", "one-point-halves-ff-129-200",
                 "asymmetric-structured-job1-64-129"):
        c = V.case(name)
        b = c.shifted_buckets(1)
        assert max(_copies(items)[0] for items in b.values()) >= 128, name  # >= 128 copies of one affine point in one bucket
        assert set(b) <= {0, 0x01, 0x80, 0xAB, 0xFF}
    # ... and in the windowed form: all entries of a (window, digit) the same point
    assert max(_copies(items)[0] for items in V.case("one-point-halves-80-129-200").windowed_buckets(1).values()) >= 200
    for name in NAMES:
        if name.startswith("plus-minus"):  # a bucket of several items that sums to the identity
            c = V.case(name)
            even = 0 if c.n[0] % 2 == 0 else 1
            b = c.shifted_buckets(even)
            assert any(bk and len(items) > 1 and sum(it[3] for it in items) % V.R == 0 for bk, items in b.items()), name
            assert c.expected_dlog(even) == 0 and c.expected_dlog(1 - even) != 0, name
            assert any(bk[1] and len(items) > 1 and sum(it[2] for it in items) % V.R == 0 for bk, items in c.windowed_buckets(even).items()), name
        if name.startswith("related"):  # two DIFFERENT inputs contribute the SAME affine point to a bucket
            c = V.case(name)
            for job in (0, 1):
                assert any(bk and _copies(items)[1] >= 2 for bk, items in c.shifted_buckets(job).items()), (name, job)
            # and an input meets the negative of another input's phi image (lambda P of input 0, -lambda P as input 6)
            b = c.shifted_buckets(1)
            assert any(bk and any((-it[3]) % V.R in {o[3] for o in items if o[0] != it[0]} for it in items) for bk, items in b.items()), name
    for c in V.all_cases():  # most slices of the counting sort empty
        for job in (0, 1):
            if c.n[job] in (1, 3):
                assert c.empty_hist_slices(job) >= 40, (c.name, job)
    assert any(c.n[j] == 1 for c in V.all_cases() for j in (0, 1)) and any(c.n[0] == 3 for c in V.all_cases())
    used = set()
    for c in V.all_cases():
        used |= set(c.shifted_buckets(1))
    assert {0, 255} <= used
    # identities with non-zero scalars, in the first and in the last lane
    c = V.case("identity-first-and-last-129-200")
    assert c.dlogs[0] is None and c.dlogs[-1] is None and c.sc[1][0] and c.sc[1][-1] and c.sc[0][0]
    assert sum(d is None for d in V.case("identity-some-64-129").dlogs) == 40


@pytest.mark.parametrize("name", NAMES)
def test_reference_group_law_matches_the_oracle_msm(name):
    """The reference is proven before any GPU run: the group law of device_ops.py, the oracle's MSM and the discrete logarithm of the
    sum (known, because every point is a known multiple of the generator) agree on both jobs of every case."""
    c = V.case(name)
    ours, theirs = V.reference_group_law(name), V.reference_oracle(name)
    assert ours == theirs, name
    for j in (0, 1):
        assert ours[j] == D.compress(V.point_of(c.expected_dlog(j))), (name, j)
    assert V.reference(name) == ours


# ---- GPU leg ---------------------------------------------------------------------------------------------------------------------------
def _small_tables_ctx(**env):
    """a context on the smallest start tables (these tests do not read them), created under extra environment settings"""
    import torch
    torch.cuda.init()
    env = dict(env, ETH_KZG_AMD_TABLE_GB="3")
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
def small_ctx():
    c = _small_tables_ctx()
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_every_form_gives_the_exact_sums(small_ctx, name):
    lib = _lib()
    c = V.case(name)
    want = V.reference(name)
    bad = []
    for form in (0, 1, 2):
        a, b, st = V.run_form(lib, small_ctx.handle, c, form)
        if (a, b) != want:
            bad.append((form, "job 0 " + ("ok" if a == want[0] else a.hex()), "job 1 " + ("ok" if b == want[1] else b.hex())))
        assert st == [0] * c.n[1], (name, form, "status words", st)  # every input is a point of the subgroup
    assert not bad, "%s: wrong sums (form, job 0, job 1): %s; expected %s %s" % (name, bad, want[0].hex(), want[1].hex())


@pytest.mark.gpu
def test_one_lane_per_point_shift_gives_the_exact_sums(tmp_path):
    """Form 2 launches four lanes per point below launch::coop_points_max and one lane per point above; the limit
    (ETH_KZG_AMD_COOP_POINTS) is read once per process, so the one-lane branch runs every case in a process of its own."""
    out = str(tmp_path / "form2.json")
    env = dict(os.environ, ETH_KZG_AMD_COOP_POINTS="0", ETH_KZG_AMD_TABLE_GB="3")
    r = subprocess.run([sys.executable, os.path.join(HERE, "verify_msm_cases.py"), "2", out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "verify-msm child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.load(open(out))
    assert sorted(got) == sorted(NAMES)
    bad = [n for n in NAMES if (bytes.fromhex(got[n][0]), bytes.fromhex(got[n][1])) != V.reference(n) or any(got[n][2])]
    assert not bad, bad


def test_the_hook_rejects_what_it_cannot_run():
    """a missing buffer is an error before the context is looked at (no GPU needed; the counts and scalars are checked in the GPU leg)"""
    lib = _lib()
    import ctypes as C
    out = C.create_string_buffer(96)
    p, s = D.compress(D.G) * 4, (1).to_bytes(32, "big") * 4
    assert lib.eth_kzg_amd_test_verify_msm(None, 0, None, 4, s, 1, s, 4, out, None) != 0
    assert lib.eth_kzg_amd_test_verify_msm(None, 0, p, 4, None, 1, s, 4, out, None) != 0
    assert lib.eth_kzg_amd_test_verify_msm(None, 0, p, 4, s, 1, s, 4, None, None) != 0


@pytest.mark.gpu
def test_the_hook_rejects_bad_counts_scalars_and_reports_bad_points(small_ctx):
    lib = _lib()
    import ctypes as C
    out = C.create_string_buffer(96)
    p, s = D.compress(D.G) * 4, (1).to_bytes(32, "big") * 4
    for form, n_pts, n0, n1 in ((3, 4, 1, 4), (-1, 4, 1, 4), (0, 4, 0, 4), (0, 4, 3, 2), (0, 3, 1, 4)):
        assert lib.eth_kzg_amd_test_verify_msm(small_ctx.handle, form, p, n_pts, s, n0, s, n1, out, None) == 3, (form, n_pts, n0, n1)
    assert lib.eth_kzg_amd_test_verify_msm(small_ctx.handle, 0, p, 4, s, 1, V.R.to_bytes(32, "big") * 4, 4, out, None) == 1
    # a curve point outside the subgroup: status 2 from every form (forms 0 and 1 decode it to the identity, as a verification would
    # have stopped there)
    import oracle_lib
    x = 5
    while True:
        cand = bytearray(x.to_bytes(48, "big"))
        cand[0] |= 0x80
        if oracle_lib.g1_validate(bytes(cand), False) == 0 and oracle_lib.g1_validate(bytes(cand), True) != 0:
            break
        x += 1
    for form in (0, 1, 2):
        st = (C.c_int32 * 4)()
        assert lib.eth_kzg_amd_test_verify_msm(small_ctx.handle, form, D.compress(D.G) * 2 + bytes(cand) + D.compress(D.G), 4, s, 2, s, 4, out, st) == 0
        assert list(st) == [0, 0, 2, 0], (form, list(st))


# ---- the same shapes through the C ABI -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def abi():
    """a default context (the byte-shifted form for every size), a context whose lincombs take the windowed form, and the batches"""
    shifted = _small_tables_ctx()
    windowed = _small_tables_ctx(ETH_KZG_AMD_PIP_SHIFT_MIN=str(1 << 20))
    blob = synth.seeded_blob(77)
    cells, proofs = shifted.compute_cells_and_kzg_proofs(blob)
    comm = shifted.blob_to_kzg_commitment(blob)
    zero = bytes(131072)
    zcells, zproofs = shifted.compute_cells_and_kzg_proofs(zero)
    zcomm = shifted.blob_to_kzg_commitment(zero)
    assert zcomm == D.compress(None) and set(zproofs) == {D.compress(None)}
    k = 37
    same = ([comm] * 200, [k] * 200, [cells[k]] * 200, [proofs[k]] * 200)
    bad_proof = (same[0], same[1], same[2], same[3][:150] + [proofs[k + 1]] + same[3][151:])
    bad_cell = (same[0], same[1], same[2][:199] + [cells[k + 1]], same[3])
    order = [0] * 128 + [1] * 128 + [2] * 10
    synth_rng = __import__("random").Random("verify-msm:abi")
    synth_rng.shuffle(order)
    ordinary = iter([3, 9, 9, 64, 65, 100, 126, 127, 0, 1])
    zz = ([], [], [], [])
    for o in order:
        if o == 2:
            j = next(ordinary)
            row = (comm, j, cells[j], proofs[j])
        else:
            j = (5, 90)[o]
            row = (zcomm, j, zcells[j], zproofs[j])
        for col, v in zip(zz, row):
            col.append(v)
    batches = {"200-copies": (same, True), "200-copies-one-proof-swapped": (bad_proof, False), "200-copies-one-cell-altered": (bad_cell, False),
               "zero-blob-2x128-and-10-ordinary": (zz, True)}
    yield shifted, windowed, batches
    shifted.close()
    windowed.close()


ABI_BATCHES = ["200-copies", "200-copies-one-proof-swapped", "200-copies-one-cell-altered", "zero-blob-2x128-and-10-ordinary"]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ABI_BATCHES)
def test_repeated_cells_verify_through_the_abi(abi, oracle, which):
    """One (commitment, index, cell, proof) many times in a batch is a valid input and must verify: every proof copy lands in the same
    buckets with r^k-weighted scalars, the commitment once with their sum.  Both forms of the lincombs, the many-problem call and three
    slices; the two forms' partial points byte for byte; the verdict from the oracle."""
    shifted, windowed, batches = abi
    args, want = batches[which]
    assert oracle.verify_cell_kzg_proof_batch(*args) is want
    n = len(args[1])
    sh = importlib.import_module("rust-eth-kzg_amd.sharding")
    bounds = [sh.shard_bounds(n, 3, r) for r in range(3)]
    for ctx in (shifted, windowed):
        assert ctx.verify_cell_kzg_proof_batch(*args) is want
        ver, st = ctx.verify_cell_kzg_proof_batch_many([args])
        assert (ver, st) == ([want], [0])
    parts = [[ctx.verify_cell_kzg_proof_batch_partial(*args, lo, hi) for lo, hi in bounds + [(0, n)]] for ctx in (shifted, windowed)]
    assert parts[0] == parts[1], [i for i in range(4) if parts[0][i] != parts[1][i]]
    for ctx, p in zip((shifted, windowed), parts):
        assert ctx.verify_cell_kzg_proof_batch_combine(p[:3]) is want
        assert ctx.verify_cell_kzg_proof_batch_combine(p[3:]) is want
