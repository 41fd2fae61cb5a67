"""The G1 subgroup test on the inputs an attacker sends: points of small order, a subgroup point plus a small-order point, the identity,
next to valid controls; and the decoders on y right at the two ends of the sign comparison and on the edges of the encoding.  The
reference of every assertion is the exact integer arithmetic of tests/small_order.py (proved in tests/test_small_order.py), never
another run of the library.

eth_kzg_amd_test_g1_decode hands out the status words AND the decoded affine coordinates behind each of the product's launch calls
(include/c_eth_kzg_test_hooks.h).  With N points in a launch and M = launch::coop_points_max() = 8192:

  device form of the subgroup test                       reached by
  k_g1_decompress_coop (four lanes per point)            forms 1 and 2, N <= M: test_every_form_every_planned_point, test_lane_and_segment_edges
  k_g1_decompress (one lane per point, check 1)          forms 1 and 2, N > M:  test_one_lane_kernels_past_the_limit
  k_g1_subgroup_coop                                     form 3, N <= M:        test_every_form_..., test_lane_and_segment_edges
  k_g1_subgroup                                          form 3, N > M:         test_one_lane_kernels_past_the_limit
  k_pip_shift_subgroup_coop (quad branch)                form 4, 2 N <= M:      test_every_form_..., test_lane_and_segment_edges;
                                                         verify_cell_kzg_proof_batch in test_public_single_routes
  k_pip_shift_subgroup (one-lane branch)                 form 4, 2 N > M:       test_one_lane_kernels_past_the_limit; tests/coop_off_check.py
  k_vm_products<VmQuad> (subgroup blocks)                test_many_verification_with_every_off_subgroup_point[small],
                                                         test_many_verification_with_a_planted_point[small]
  k_vm_products<VmLane> (one-lane subgroup blocks)       tests/coop_off_check.py (ETH_KZG_AMD_COOP_POINTS=0, run by tests/test_gpu_parity.py):
                                                         the same pass, asserted to be short-chain
  the decoder without the test (k_g1_decompress, check 0): form 0 and the decode of forms 3 and 4 -- every boundary-y and encoding-edge point

The six forms behind the hook are given all of small_order.g1_cases(): every +-S_l, the composite-order points, [k]G + S_l, the identity,
the valid controls, every boundary-y point in both sign encodings and every encoding edge.  The two k_vm_products forms take their points
from a many-verification's problems: small_order.many_plan gives one pass every +-S_l, both composite-order points and every [k]G + S_l,
each as a proof and as a commitment, the identity and valid problems; the boundary-y points and the encoding edges are the decoders' matter (the
hook's forms) and are not planted in a many-verification.

In the product, launch::g1_subgroup2 has no caller that runs: verify.hip takes it only on a second stream that no setting switches on
(Engine::v_two_streams_ is constant false).  Hook form 3 is the one way to it, so there is no public-route case for it below.

What a refused slot holds: the decoders write the identity (96 zero bytes) over a point they refuse, so forms 0, 1 and 2 leave zero bytes
for every refused point, and so does the decode of forms 3 and 4 for status 1.  The subgroup-only kernels of forms 3 and 4 take the point
array read-only and write the status word alone: a point they refuse with 2 keeps its decoded coordinates, and the test asserts exactly
those (the verifiers read the status words before they use any sum)."""
import importlib
import os

import ctypes as C
import pytest

import oracle_lib
import small_order as so
import synth
from many_coop_off_check import many_sums

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu
COOP_POINTS_MAX = 8192
G1_ERROR = "CouldNotDeserializeG1Point"
COUNTS = [1, 15, 16, 17, 63, 64, 65]
SPLITS = [(1, 1), (16, 1), (15, 17), (64, 1)]
BIG_L = 52437899


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


def decode(ctx, form, encs, n0=None):
    """eth_kzg_amd_test_g1_decode over the segments [n0 | rest] -> (status list, [96 bytes] list)"""
    n = len(encs)
    n0 = n if n0 is None else n0
    st = (C.c_int32 * n)()
    xy = C.create_string_buffer(96 * n)
    rc = kzg.load_library().eth_kzg_amd_test_g1_decode(ctx.handle, form, b"".join(encs), n0, n - n0, st, xy)
    assert rc == 0, (form, n0, n - n0, rc)
    return list(st), [xy.raw[96 * i:96 * i + 96] for i in range(n)]


def want(case, form):
    """(status, 96 bytes) the exact integers plan for a case behind the launches of a form"""
    if form == 0:
        return case.status0, case.xy0
    if form in (1, 2):
        return case.status1, case.xy1
    return case.status1, case.xy0  # forms 3 and 4: decoded without the test, then the status word alone is written


def check(ctx, form, cases, n0=None, tag=""):
    st, xy = decode(ctx, form, [c.enc for c in cases], n0)
    bad = [(i, c.name, st[i], want(c, form)[0]) for i, c in enumerate(cases) if st[i] != want(c, form)[0]]
    assert not bad, "form %d %s: (slot, case, status, planned) %s" % (form, tag, bad[:12])
    bad = [(i, c.name, xy[i][:48] == want(c, form)[1][:48], xy[i][48:] == want(c, form)[1][48:])
           for i, c in enumerate(cases) if xy[i] != want(c, form)[1]]
    assert not bad, "form %d %s: (slot, case, x equal, y equal) %s" % (form, tag, bad[:12])
    return st, xy


@pytest.mark.parametrize("form", [0, 1, 2, 3, 4])
def test_every_form_every_planned_point(ctx, form):
    cases = so.g1_cases()
    assert len(cases) == so.N_G1_CASES and 2 * len(cases) <= COOP_POINTS_MAX  # forms 1 .. 4: the four-lane kernels
    st, xy = check(ctx, form, cases, None if form <= 1 else 40)
    by = {c.name: (s, v) for c, s, v in zip(cases, st, xy)}
    # the sign: a boundary-y point and its flipped encoding decode to the same x and to y and p - y
    seen = 0
    for label, pt in so.boundary_points():
        for name, y in ((label, pt[1]), (label + " flipped", so.P - pt[1])):
            s, v = by[name]
            if s == 0 or form >= 3:
                assert v == pt[0].to_bytes(48, "big") + y.to_bytes(48, "big"), (form, name)
                seen += 1
            else:
                assert s == 2 and v == bytes(96), (form, name)
    assert seen == (36 if form in (0, 3, 4) else 0)  # (they are off the subgroup: forms 1 and 2 refuse them and write the identity)
    if form:
        assert sum(s == 2 for s in st) == sum(c.status1 == 2 for c in cases) >= 22 + 36


def _alternating(n, bad_at_even, bad_pool, good_pool):
    out = []
    for i in range(n):
        pool = bad_pool if (i % 2 == 0) == bad_at_even else good_pool
        out.append(pool[i // 2 % len(pool)])
    return out


def _pools(form):
    cases = so.g1_cases()
    good = [c for c in cases if c.status1 == 0 and c.point is not None]
    off = [c for c in cases if c.status1 == 2]
    junk = [c for c in cases if c.status0 == 1]
    assert len(good) == 5 and len(off) >= 46 and len(junk) >= 20
    if form == 0:  # no subgroup test: only an undecodable point is refused
        return good, junk, junk
    mixed = [x for pair in zip(off, junk * 3) for x in pair]  # status 2 and status 1 in turn
    return good, mixed, off


@pytest.mark.parametrize("form", [0, 1, 2, 3, 4])
def test_lane_and_segment_edges(ctx, form):
    """16 points per block of the four-lane kernels, 64 per wave of the one-lane ones: counts around both, a refused point first and last
    (the padding lanes behind the last point repeat it), neighbours alternating so that no two adjacent statuses agree"""
    good, bad, off = _pools(form)
    junk = [c for c in so.g1_cases() if c.status0 == 1]
    for n in COUNTS:
        for bad_at_even in (True, False):
            cases = _alternating(n, bad_at_even, bad, good)
            st, _ = check(ctx, form, cases, tag="n = %d" % n)
            assert all(a != b for a, b in zip(st, st[1:])), (form, n, st)
            assert (st[0] != 0) == bad_at_even and (st[-1] != 0) == (bad_at_even == (n % 2 == 1))
    if form <= 1:
        return  # one segment
    for n0, n1 in SPLITS:
        for swap in (False, True):  # the last entry of segment 0 and the first of segment 1 both refused, with different statuses
            k0, k1 = (junk, off) if swap else (off, junk)
            seg0 = [(k0[i % len(k0)] if (n0 - 1 - i) % 2 == 0 else good[i % 5]) for i in range(n0)]
            seg1 = [(k1[i % len(k1)] if i % 2 == 0 else good[i % 5]) for i in range(n1)]
            st, _ = check(ctx, form, seg0 + seg1, n0, tag="split (%d, %d)" % (n0, n1))
            assert st[n0 - 1] != 0 and st[n0] != 0
            assert all(a != b for a, b in zip(st, st[1:])), (form, n0, n1, st)


@pytest.mark.parametrize("form", [1, 2, 3, 4])
def test_one_lane_kernels_past_the_limit(ctx, form):
    """the same list repeated past coop_points_max(): one launch per form takes the one-lane kernel, and every status and coordinate
    equals the small launch's (and the plan), element for element"""
    cases = so.g1_cases()
    reps = COOP_POINTS_MAX // len(cases) + 1
    n = reps * len(cases)
    assert COOP_POINTS_MAX < n < COOP_POINTS_MAX + len(cases)
    small = decode(ctx, form, [c.enc for c in cases], None if form == 1 else 40)
    big = check(ctx, form, cases * reps, None if form == 1 else 4001, tag="%d points" % n)
    assert big[0] == small[0] * reps and big[1] == small[1] * reps


# ---- the public routes ---------------------------------------------------------------------------------------------------------------------
PLANTS = [(l, mixed) for l in (3, BIG_L) for mixed in (False, True)]  # S_l and [k]G + S_l


@pytest.fixture(scope="module")
def material(ctx):
    blobs = [synth.seeded_blob(11), synth.seeded_blob(12)]
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(blobs)
    assert st == [0, 0]
    comms = [ctx.blob_to_kzg_commitment(b) for b in blobs]
    return blobs, comms, cells, proofs


def _cell_problem(material, b, first, n=8):
    _, comms, cells, proofs = material
    idx = list(range(first, first + n))
    return [comms[b]] * n, idx, [cells[b][i] for i in idx], [proofs[b][i] for i in idx]


def _plant(problem, enc, role, at):
    comm, idx, cells, proofs = (list(x) for x in problem)
    (proofs if role == "proof" else comm)[at] = enc
    return comm, idx, cells, proofs


def _single_cell_route(c, material, oracle, tag):
    good = _cell_problem(material, 0, 40)
    assert c.verify_cell_kzg_proof_batch(*good) is True and oracle.verify_cell_kzg_proof_batch(*good) is True, tag
    for l, mixed in PLANTS:
        for role in ("proof", "commitment"):
            p = _plant(good, so.planted(l, mixed).enc, role, 5)
            with pytest.raises(oracle_lib.OracleError) as e:
                oracle.verify_cell_kzg_proof_batch(*p)
            assert e.value.code == 2  # ORACLE_ERR_G1: exactly where the oracle refuses
            with pytest.raises(kzg.KzgError, match=G1_ERROR):
                c.verify_cell_kzg_proof_batch(*p)
    assert c.verify_cell_kzg_proof_batch(*good) is True, tag  # and nothing is left behind


def test_public_single_routes(ctx, material, oracle):
    blobs, comms, _, _ = material
    _single_cell_route(ctx, material, oracle, "default settings")
    z = (0x1234567).to_bytes(32, "big")
    proof, y = ctx.compute_kzg_proof(blobs[0], z)
    bproof = ctx.compute_blob_kzg_proof(blobs[0], comms[0])
    assert ctx.verify_kzg_proof(comms[0], z, y, proof) is True and ctx.verify_blob_kzg_proof(blobs[0], comms[0], bproof) is True
    for l, mixed in PLANTS:
        enc = so.planted(l, mixed).enc
        for args in ((enc, z, y, proof), (comms[0], z, y, enc)):
            with pytest.raises(kzg.KzgError, match=G1_ERROR):
                ctx.verify_kzg_proof(*args)
            with pytest.raises(oracle_lib.OracleError) as e:
                oracle.verify_kzg_proof(*args)
            assert e.value.code == 2
        for args in ((blobs[0], enc, bproof), (blobs[0], comms[0], enc)):
            with pytest.raises(kzg.KzgError, match=G1_ERROR):
                ctx.verify_blob_kzg_proof(*args)
    assert ctx.verify_kzg_proof(comms[0], z, y, proof) is True and ctx.verify_blob_kzg_proof(blobs[0], comms[0], bproof) is True


@pytest.mark.parametrize("pip_shift_min", [1, 1 << 20])
def test_cell_verification_under_either_msm_form(material, oracle, pip_shift_min):
    """ETH_KZG_AMD_PIP_SHIFT_MIN is read when a context is made: 1 = the byte-shifted form (g1_decode2 + pip_shift_prepare_and_subgroup; also
    the default), a value above the batch = the windowed form, whose points come through g1_decompress2.  (There is no third way: the
    second-stream route through g1_subgroup2 cannot be switched on in the product; the hook's form 3 reaches that launcher.)"""
    c = _ctx(ETH_KZG_AMD_PIP_SHIFT_MIN=str(pip_shift_min))
    try:
        _single_cell_route(c, material, oracle, "PIP_SHIFT_MIN=%d" % pip_shift_min)
    finally:
        c.close()


@pytest.mark.parametrize("form", ["small", "regular"])
def test_many_verification_with_a_planted_point(material, form):
    """12 problems of 8 cells, one of them carrying the planted point.  A pass of at most 2 x host threads problems takes the short-chain
    form (verify_many.hip: vm_small_max_ = -1), whose scalar multiplications run in the launch of the subgroup tests, on points not yet
    known to be bad: ETH_KZG_AMD_HOST_THREADS=8 gives it, =2 the regular, folded form.  The planted problem is refused alone; every other
    problem's verdict, status and pair of sums are those of the same call with that problem valid."""
    threads = 8 if form == "small" else 2
    c = _ctx(ETH_KZG_AMD_HOST_THREADS=str(threads))
    try:
        problems = [_cell_problem(material, b % 2, 8 * (b // 2)) for b in range(12)]
        wrong = list(problems[9][3])
        wrong[0] = problems[8][3][0]
        problems[9] = (problems[9][0], problems[9][1], problems[9][2], wrong)  # a neighbour whose verdict is False
        rc, base = many_sums(c, problems)
        assert rc == 0 and base.status == [0] * 12 and base.verified == [b != 9 for b in range(12)]
        assert (base.small, base.folded) == (form == "small", form == "regular")
        for l, mixed in PLANTS:
            for role in ("proof", "commitment"):
                planted = list(problems)
                planted[4] = _plant(problems[4], so.planted(l, mixed).enc, role, 3)
                rc, got = many_sums(c, planted)
                tag = (form, l, mixed, role)
                assert rc == 0 and (got.small, got.folded) == (base.small, base.folded), tag
                assert got.status == [2 if b == 4 else 0 for b in range(12)], (tag, got.status)
                assert got.verified == [b not in (4, 9) for b in range(12)], (tag, got.verified)
                assert [got.sums[b] for b in range(12) if b != 4] == [base.sums[b] for b in range(12) if b != 4], tag
                if got.folded:
                    assert got.rho[4] == 0 and all(got.rho[b] != 0 for b in range(12) if b != 4), tag
                assert c.verify_cell_kzg_proof_batch_many(planted) == (got.verified, got.status), tag
    finally:
        c.close()


@pytest.mark.parametrize("form", ["small", "regular"])
def test_many_verification_with_every_off_subgroup_point(material, oracle, form):
    """One pass whose proof and commitment slots hold every +-S_l, both composite-order points and every [k]G + S_l (each once as a proof
    and once as a commitment, spread over six problems), the identity (a whole valid problem of it, and in the place of one proof) and
    valid controls: small_order.many_plan.  In the short-chain form these are the inputs of k_vm_products<VmQuad>'s subgroup blocks
    (tests/coop_off_check.py gives the same pass to k_vm_products<VmLane>).  Status and verdict of every problem are the plan's; the
    well-formed problems' verdicts are the oracle's; the pairs of sums of the problems next to the refused ones do not change."""
    c = _ctx(ETH_KZG_AMD_HOST_THREADS="8" if form == "small" else "2")
    try:
        base, planted = so.many_plan([_cell_problem(material, b % 2, 8 * (b // 2)) for b in range(12)])
        live = [b for b in range(12) if b not in so.MANY_PLANTED]
        for b in live:
            assert oracle.verify_cell_kzg_proof_batch(*planted[b]) is so.MANY_VERDICTS[b], b
        for b in so.MANY_PLANTED:
            with pytest.raises(oracle_lib.OracleError) as e:
                oracle.verify_cell_kzg_proof_batch(*planted[b])
            assert e.value.code == 2
        rc, ref = many_sums(c, base)
        assert rc == 0 and ref.status == [0] * 12 and ref.verified == [b not in (7, 9) for b in range(12)], (ref.status, ref.verified)
        rc, got = many_sums(c, planted)
        assert rc == 0 and (got.small, got.folded) == (ref.small, ref.folded) == (form == "small", form == "regular")
        assert got.status == so.MANY_STATUS, got.status
        assert got.verified == so.MANY_VERDICTS, got.verified
        assert [got.sums[b] for b in live] == [ref.sums[b] for b in live]
        if got.folded:
            assert [got.rho[b] == 0 for b in range(12)] == [b in so.MANY_PLANTED for b in range(12)]
        assert c.verify_cell_kzg_proof_batch_many(planted) == (got.verified, got.status)
    finally:
        c.close()


def test_point_and_blob_many_with_a_planted_point(ctx, material):
    blobs, comms, _, _ = material
    zs = [(0x1000 + 77 * i).to_bytes(32, "big") for i in range(9)]
    items, bitems = [], []
    for i, z in enumerate(zs):
        proof, y = ctx.compute_kzg_proof(blobs[i % 2], z)
        items.append((comms[i % 2], z, y, proof))
        bitems.append((blobs[i % 2], comms[i % 2], ctx.compute_blob_kzg_proof(blobs[i % 2], comms[i % 2])))
    items[6] = (items[6][0], items[6][1], items[6][2], items[5][3])  # wrong proofs: neighbours whose verdict is False
    bitems[6] = (bitems[6][0], bitems[6][1], bitems[5][2])
    want_ver = [i != 6 for i in range(9)]
    assert ctx.verify_kzg_proof_many(items) == (want_ver, [0] * 9)
    assert ctx.verify_blob_kzg_proof_many(bitems) == (want_ver, [0] * 9)
    for l, mixed in PLANTS:
        enc = so.planted(l, mixed).enc
        for at in (0, 5, 8):
            for role in (0, 3):
                it = list(items)
                it[at] = tuple(enc if j == role else v for j, v in enumerate(items[at]))
                ver, st = ctx.verify_kzg_proof_many(it)
                assert st == [2 if i == at else 0 for i in range(9)], (l, mixed, at, role, st)
                assert ver == [want_ver[i] and i != at for i in range(9)], (l, mixed, at, role, ver)
            for role in (1, 2):
                it = list(bitems)
                it[at] = tuple(enc if j == role else v for j, v in enumerate(bitems[at]))
                ver, st = ctx.verify_blob_kzg_proof_many(it)
                assert st == [2 if i == at else 0 for i in range(9)], (l, mixed, at, role, st)
                assert ver == [want_ver[i] and i != at for i in range(9)], (l, mixed, at, role, ver)
