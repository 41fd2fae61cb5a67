"""The data columns of one block, the commitments given once: eth_kzg_amd_verify_data_columns / _device.

Column j of a call is the problem tests/data_columns.py expands it into, so every check here is against the EXPANDED input: verdicts
from the CPU oracle, verdicts and statuses from eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex, and -- through the hook
eth_kzg_amd_test_verify_data_columns_sums, a tap on the pass's own read-backs -- every leaf, digest, per-column pair, weight, folded
pair and probe byte for byte: against the statement in hashlib and Python integers (tests/many_leaf.py, tests/verify_transcript.py) and
against the tap of the expanded pass (eth_kzg_amd_test_verify_many_sums_ex, which tests/test_gpu_many_leaf.py and
tests/test_verify_inputs.py hold to that statement).  The tap's counts tell the column pass from a forward to _many: n_u commitment
points decoded per pass and n + Bc n_u + Bc scalar multiplications, where the expanded pass has Bc n_u and 2 n + Bc n_u.
The context is test_verify_inputs.py's many_ctx: small tables, two host threads -- the short-chain form up to 4 columns, the fold above,
per-problem checks from 4 suspects.  Blobs come from the library's prover: 129 seeded ones and the zero blob."""
import ctypes as C
import importlib
import os
import threading

import numpy as np
import pytest

import data_columns as D
import many_leaf as M
import small_order as S
import synth
import vectors
import verify_transcript as T

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu

LEAF = 1  # ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT
HOST_THREADS = T.MANY_HOST_THREADS
N_SEEDED, ZERO = 129, 129  # material: blobs 0 .. 128 seeded, blob 129 the zero blob (identity commitment, identity proofs)
INF = T.INF
_expanded = {}  # the expanded pass's tap and the statement, computed once per case, shared by the ways, never changed


def _ctx(devices=None, **env):
    import torch
    torch.cuda.init()
    env = dict(env, ETH_KZG_AMD_TABLE_GB="3")  # the start tables: results never depend on the table
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return kzg.DASContext(use_precomp=True, devices=devices)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    c = _ctx(ETH_KZG_AMD_HOST_THREADS=str(HOST_THREADS))
    yield c
    c.close()


class Mat:
    pass


@pytest.fixture(scope="module")
def mat(ctx):
    blobs = [synth.seeded_blob(7300 + i) for i in range(N_SEEDED)] + [bytes(131072)]
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(blobs)
    assert st == [0] * len(blobs)
    m = Mat()
    m.commitments, m.cells, m.proofs = [ctx.blob_to_kzg_commitment(b) for b in blobs], cells, proofs
    assert m.commitments[ZERO] == INF and set(m.proofs[ZERO]) == {INF} and len(set(m.commitments)) == len(blobs)
    return m


def _block(mat, picks, indices):
    return D.block(mat.commitments, mat.cells, mat.proofs, picks, indices)


class Dev:
    """the three byte arrays of a column call in device memory, `shift` bytes into their allocations"""

    def __init__(self, call, shift=0, stream=None):
        import torch
        self.n_blobs, self.indices = len(call[0]), call[1]
        self.keep, self.ptrs = [], []
        for raw in D.flat_bytes(call[0], call[2], call[3]):
            a = np.frombuffer(raw or bytes(1), dtype=np.uint8)
            if stream is None:
                d = torch.empty(shift + len(a), dtype=torch.uint8, device="cuda")
                d[shift:].copy_(torch.from_numpy(a.copy()))
            else:  # asynchronous copies on the caller's stream, from pinned memory: the call must wait for them
                pinned = torch.from_numpy(a.copy()).pin_memory()
                with torch.cuda.stream(stream):
                    d = torch.empty(shift + len(a), dtype=torch.uint8, device="cuda")
                    d[shift:].copy_(pinned, non_blocking=True)
                self.keep.append(pinned)
            self.keep.append(d)
            self.ptrs.append(d.data_ptr() + shift)
        if stream is None:
            torch.cuda.synchronize()

    def run(self, ctx, leaf, stream=None):
        return ctx.verify_data_columns_device(self.n_blobs, self.ptrs[0], self.indices, self.ptrs[1], self.ptrs[2], stream=stream, leaf_transcript=leaf)


class Sums:
    pass


def _unpack(nb, n_cells, ver, st, form, sums, rho, fold, pr, ps, npr, dig, leaves, max_probes):
    out = Sums()
    out.verified, out.status = [bool(v) for v in ver], list(st)
    out.small, out.folded, out.searched, out.fold_verdict = bool(form[0]), bool(form[1]), bool(form[2]), form[3]
    out.sums = [sums.raw[96 * b:96 * b + 96] for b in range(nb)]
    out.rho = [sum(rho[4 * b + j] << (32 * j) for j in range(4)) for b in range(nb)]
    out.fold, out.n_probes = fold.raw, npr.value
    out.probes = [(pr[3 * q], pr[3 * q + 1], ps.raw[96 * q:96 * q + 96], bool(pr[3 * q + 2])) for q in range(min(npr.value, max_probes))]
    out.digests = [dig.raw[32 * b:32 * b + 32] for b in range(nb)]
    out.leaves = [leaves.raw[32 * k:32 * k + 32] for k in range(n_cells)]
    return out


def _buffers(nb, n_cells, max_probes):
    return ((C.c_int32 * nb)(), (C.c_int32 * nb)(), (C.c_int32 * 4)(), C.create_string_buffer(96 * nb), (C.c_uint32 * (4 * nb))(),
            C.create_string_buffer(96), (C.c_int32 * (3 * max_probes))(), C.create_string_buffer(96 * max_probes), C.c_uint64(0),
            C.create_string_buffer(32 * nb), C.create_string_buffer(32 * max(1, n_cells)))


def column_sums(ctx, call, where, flags, max_probes=64):
    """eth_kzg_amd_test_verify_data_columns_sums -> (return code, Sums with .counts = (commitments decoded, multiplications))"""
    lib = kzg.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nb, nc = len(call[0]), len(call[1])
    ver, st, form, sums, rho, fold, pr, ps, npr, dig, leaves = bufs = _buffers(nc, nb * nc, max_probes)
    counts = (C.c_uint64 * 2)()
    tail = (flags, ver, st, form, sums, rho, fold, pr, ps, max_probes, C.byref(npr), dig, leaves, counts)
    if where == "host":
        _, _, ca, idx, cla, pa, _keep = ctx._marshal_columns(*call)
        rc = lib.eth_kzg_amd_test_verify_data_columns_sums(ctx.handle, nb, 0, vp(ca), nc, vp(idx), vp(cla), vp(pa), *tail)
    else:
        d = Dev(call)
        idx = np.array(call[1], dtype=np.uint64)
        rc = lib.eth_kzg_amd_test_verify_data_columns_sums(ctx.handle, nb, 1, C.c_void_p(d.ptrs[0]), nc, vp(idx), C.c_void_p(d.ptrs[1]),
                                                           C.c_void_p(d.ptrs[2]), *tail)
    out = _unpack(nc, nb * nc, *bufs, max_probes)
    out.counts = (counts[0], counts[1])
    return rc, out


def expanded_sums(ctx, problems, flags, max_probes=64):
    """eth_kzg_amd_test_verify_many_sums_ex on the expanded problems (host form)"""
    lib = kzg.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nb, n_cells = len(problems), sum(len(p[1]) for p in problems)
    bufs = _buffers(nb, n_cells, max_probes)
    ver, st, form, sums, rho, fold, pr, ps, npr, dig, leaves = bufs
    _, lens, tabs, _keep = ctx._marshal_many(problems)
    rc = lib.eth_kzg_amd_test_verify_many_sums_ex(ctx.handle, nb, vp(lens[0]), vp(tabs[0]), vp(lens[1]), vp(tabs[1]), vp(lens[2]), vp(tabs[2]),
                                                  vp(lens[3]), vp(tabs[3]), flags, ver, st, form, sums, rho, fold, pr, ps, max_probes, C.byref(npr), dig, leaves)
    return rc, _unpack(nb, n_cells, *bufs, max_probes)


def _swap(col, i, j):
    out = list(col)
    out[i], out[j] = out[j], out[i]
    return out


def _negated(proof):
    assert proof != INF
    return bytes([proof[0] ^ 0x20]) + proof[1:]  # the sign bit of a compressed point: the other y


# ---- the cases: (picks of blobs, column indices, what is done to the call, columns that must come out wrong) ---------------------------------
def _cases(mat):
    """name -> (call, wrong columns, form (small, folded, searched) or None, statement: also held to the Python statement)"""
    out = {}

    def add(name, picks, indices, wrong=(), change=None, form=None, statement=False):
        call = _block(mat, picks, indices)
        if change:
            change(call)
        out[name] = (call, set(wrong), form, statement)

    short, folded, searched = (True, False, False), (False, True, False), (False, True, True)
    # shapes: n_blobs 1, 2, 3, 64, 65, 128, 129 (129 crosses the 128 lanes of a reduction half); n_columns 1 (no fold), 2, 3, 5 (above the
    # short-chain bound of 4), 6 with one wrong (the fold with a search); indices 0, 1, 64, 127, descending, the same index twice
    add("1x1-index-0", [0], [0], form=short, statement=True)
    add("2x2-descending", [0, 1], [1, 0], form=short, statement=True)
    add("3x3-indices-127-64-1", [0, 1, 2], [127, 64, 1], form=short, statement=True)
    add("64x2", list(range(64)), [0, 1], form=short)
    add("65x1", list(range(65)), [64], form=short)
    add("128x3", list(range(128)), [127, 1, 0], form=short)
    add("129x2-same-index-twice", list(range(129)), [5, 5], form=short)
    add("3x5-folded", [2, 1, 0], [127, 64, 1, 0, 64], form=folded, statement=True)
    add("129x5-folded", list(range(129)), [127, 126, 1, 0, 64], form=folded)
    add("2x6-search", [0, 1], [0, 1, 64, 127, 3, 2], wrong=[4], change=lambda c: c[3].__setitem__(4, _swap(c[3][4], 0, 1)), form=searched, statement=True)
    # valid and degenerate inputs
    add("zero-blob", [ZERO], [0, 1, 127], form=short, statement=True)
    add("zero-blob-folded", [ZERO, ZERO], [1, 0, 127, 64, 2], form=folded)
    add("all-blobs-equal", [3, 3, 3, 3], [1, 0], form=short, statement=True)
    add("two-equal-among-different", [4, 5, 4, 6, 7], [127, 1, 0, 64, 9], form=folded)
    add("identity-commitment-next-to-others", [8, ZERO, 9], [0, 1, 64], form=short, statement=True)
    # wrong inputs: one column wrong among valid ones
    add("two-proofs-swapped", [0, 1, 2], [0, 1, 64, 127, 5], wrong=[1], change=lambda c: c[3].__setitem__(1, _swap(c[3][1], 0, 2)), form=searched)
    add("proof-replaced-by-identity", [0, 1, 2], [0, 1, 64], wrong=[2], change=lambda c: c[3][2].__setitem__(1, INF), form=short, statement=True)
    add("proof-replaced-by-its-negative", [0, 1, 2], [1, 0, 64], wrong=[0], change=lambda c: c[3][0].__setitem__(2, _negated(c[3][0][2])), form=short)
    add("one-cell-byte-changed", [0, 1], [0, 1, 64, 127, 2], wrong=[3],
        change=lambda c: c[2][3].__setitem__(1, c[2][3][1][:2047] + bytes([c[2][3][1][2047] ^ 1])), form=searched)

    def misfile(c):  # column 1's cells and proofs filed under the neighbouring index
        c[1][1] = c[1][1] + 1
    add("filed-under-a-neighbouring-index", [0, 1, 2], [0, 64, 127], wrong=[1], change=misfile, form=short)

    def all_wrong(c):
        for j in range(len(c[1])):
            c[3][j] = _swap(c[3][j], 0, 1)
    add("every-column-wrong", [0, 1], [0, 1, 2, 3, 4, 5], wrong=range(6), change=all_wrong, form=searched)
    return out


CASE_NAMES = ["1x1-index-0", "2x2-descending", "3x3-indices-127-64-1", "64x2", "65x1", "128x3", "129x2-same-index-twice", "3x5-folded", "129x5-folded",
              "2x6-search", "zero-blob", "zero-blob-folded", "all-blobs-equal", "two-equal-among-different", "identity-commitment-next-to-others",
              "two-proofs-swapped", "proof-replaced-by-identity", "proof-replaced-by-its-negative", "one-cell-byte-changed",
              "filed-under-a-neighbouring-index", "every-column-wrong"]


@pytest.fixture(scope="module")
def cases(mat):
    c = _cases(mat)
    assert list(c) == CASE_NAMES
    return c


def _reference(ctx, oracle, name, call, flags, statement):
    """the expanded pass: its tap on this build, the oracle's verdicts, and (small cases) the statement in hashlib and Python integers"""
    key = (name, flags)
    if key not in _expanded:
        problems = D.expand(*call)
        rc, tap = expanded_sums(ctx, problems, flags)
        assert rc == 0
        if name not in _expanded:
            _expanded[name] = [oracle.verify_cell_kzg_proof_batch(*p) for p in problems]
        verdicts = _expanded[name]
        stated = None
        if statement:
            on = [True] * len(problems)
            if flags:
                digests, sums, rho, fold = M.pass_statement(problems, on, on, tap.folded)
                leaves = M.pass_leaves(problems, on)
            else:
                digests = [T.cell_digest(*p) for p in problems]
                sums = [T.cell_partial(*p, 0, len(p[1]), r=T.reduce_digest(d)) for p, d in zip(problems, digests)]
                rho = T.fold_weights(digests, on)
                fold, leaves = (T.fold_pair(sums, rho, 0, len(sums)) if tap.folded else None), None
            stated = (digests, sums, rho, fold, leaves)
        _expanded[key] = (problems, tap, verdicts, stated)
    return _expanded[key]


WAYS = {"host": ("host", 0), "host-leaf": ("host", LEAF), "device": ("device", 0), "device-leaf": ("device", LEAF)}


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_a_column_pass_equals_the_expanded_pass_byte_for_byte(ctx, oracle, cases, name, way):
    where, flags = WAYS[way]
    call, wrong, form, statement = cases[name]
    nb, nc = len(call[0]), len(call[1])
    problems, ref, verdicts, stated = _reference(ctx, oracle, name, call, flags, statement)
    assert verdicts == [j not in wrong for j in range(nc)], (name, verdicts)  # the oracle names exactly the columns made wrong
    assert (ref.verified, ref.status) == (verdicts, [0] * nc), name
    rc, got = column_sums(ctx, call, where, flags)
    assert rc == 0, (name, way, rc)
    assert (got.verified, got.status) == (verdicts, [0] * nc), (name, way, got.verified, got.status)
    assert (got.small, got.folded, got.searched) == (ref.small, ref.folded, ref.searched) == form, (name, way, got.small, got.folded, got.searched)
    assert got.digests == ref.digests, (name, way)
    bad = [(j, got.sums[j][:48] == ref.sums[j][:48], got.sums[j][48:] == ref.sums[j][48:]) for j in range(nc) if got.sums[j] != ref.sums[j]]
    assert not bad, "%s %s: (column, A equal, B equal) %s" % (name, way, bad)
    assert 0xff not in {s[0] for s in got.sums}  # no slot still holds its poison
    assert got.fold == ref.fold and got.fold_verdict == ref.fold_verdict, (name, way)
    if got.folded:  # (a pass that is not folded computes no weights)
        assert got.rho == ref.rho, (name, way)
    assert got.n_probes == ref.n_probes and got.probes == ref.probes, (name, way)
    if flags:
        assert got.leaves == ref.leaves, (name, way, [k for k in range(nb * nc) if got.leaves[k] != ref.leaves[k]][:10])
    # a column pass, not a forward to _many: the unique commitments once, n + Bc n_u + Bc products (the expanded pass: Bc n_u, 2 n + Bc n_u)
    n_u = len(set(call[0]))
    assert got.counts == D.counts(nb * nc, nc, n_u), (name, way, got.counts)
    if stated:
        digests, sums, rho, fold, leaves = stated
        assert got.digests == digests and got.sums == sums, (name, way)
        if got.folded:
            assert got.rho == rho and got.fold == fold, (name, way)
            live = [True] * nc
            plan = T.search_plan(live, verdicts, HOST_THREADS) if got.searched else []
            assert [(lo, hi, ok) for lo, hi, _, ok in got.probes] == plan, (name, way)
            assert all(raw == T.fold_pair(sums, rho, lo, hi) for lo, hi, raw, _ in got.probes), (name, way)
        if leaves is not None:
            assert got.leaves == leaves, (name, way)


def test_edge_values_of_h64(ctx, cases):
    """column index 0: h^64 = 1, so B - (commitment side) = A; index 1: brp7 = 64, h^64 = -1.  With the zero blob the commitment side and
    the interpolation vanish as well (identity commitment, zero cells) and A is the identity: both sums are the identity, exactly"""
    call = cases["zero-blob"][0]
    for where in ("host", "device"):
        rc, got = column_sums(ctx, call, where, LEAF)
        assert rc == 0 and got.sums == [INF + INF] * 3 and got.verified == [True] * 3, where


# ---- the public calls -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x3-indices-127-64-1", "129x5-folded", "2x6-search", "zero-blob-folded", "two-equal-among-different",
                                  "proof-replaced-by-its-negative", "every-column-wrong"])
def test_the_public_calls_agree_with_many_ex_on_the_expanded_input(ctx, cases, name):
    call, wrong, _, _ = cases[name]
    nc = len(call[1])
    want = ([j not in wrong for j in range(nc)], [0] * nc)
    problems = D.expand(*call)
    d = Dev(call)
    for leaf in (False, True):
        assert ctx.verify_cell_kzg_proof_batch_many(problems, leaf_transcript=leaf) == want, (name, leaf)
        assert ctx.verify_data_columns(*call, leaf_transcript=leaf) == want, (name, leaf)
        assert d.run(ctx, leaf) == want, (name, leaf)


def _both(ctx, call, want):
    problems = D.expand(*call)
    d = Dev(call)
    for leaf in (False, True):
        assert ctx.verify_cell_kzg_proof_batch_many(problems, leaf_transcript=leaf) == want, ("expanded", leaf)
        assert ctx.verify_data_columns(*call, leaf_transcript=leaf) == want, ("host", leaf)
        assert d.run(ctx, leaf) == want, ("device", leaf)


def test_statuses_in_the_reference_order(ctx, mat):
    r_be = T.R.to_bytes(32, "big")
    # a bad commitment marks ALL columns 2, also next to a column with a bad proof or a bad cell; an index >= 128 is 3 ahead of everything
    call = _block(mat, [0, 1, 2], [0, 128, 64, 127, 1 << 40])
    call[0][1] = T.off_subgroup_point()
    call[3][2][0] = T.off_subgroup_point()
    call[2][3][2] = call[2][3][2][:-32] + r_be
    _both(ctx, call, ([False] * 5, [2, 3, 2, 2, 3]))
    # without the bad commitment: the bad proof is 2 and the non-canonical cell 1, each in its own column; the others verify
    call = _block(mat, [0, 1, 2], [0, 128, 64, 127, 5])
    call[3][2][0] = T.off_subgroup_point()
    call[2][3][2] = call[2][3][2][:-32] + r_be
    _both(ctx, call, ([True, False, False, False, True], [0, 3, 2, 1, 0]))
    # a bad proof AND a bad cell in one column: the proof is reported (commitments, proofs, cells)
    call = _block(mat, [0, 1], [7, 8, 9, 10, 11])
    call[3][4][1] = T.off_subgroup_point()
    call[2][4][0] = r_be + call[2][4][0][32:]
    _both(ctx, call, ([True] * 4 + [False], [0, 0, 0, 0, 2]))


def test_small_order_points_as_commitment_and_as_proof(ctx, mat):
    for l, pt in S.small_order_points().items():
        enc = S.encode(pt)
        as_commitment = _block(mat, [0, 1], [0, 1, 2])
        as_commitment[0][0] = enc
        _both(ctx, as_commitment, ([False] * 3, [2] * 3))
        as_proof = _block(mat, [0, 1], [0, 1, 2, 3, 4])
        as_proof[3][3][1] = enc
        _both(ctx, as_proof, ([True, True, True, False, True], [0, 0, 0, 2, 0]))


def _invalid(res):
    lib = kzg.load_library()
    assert res.status == 1 and res.error_msg
    msg = C.string_at(res.error_msg).decode()
    lib.eth_kzg_free_error_message(res.error_msg)
    assert msg.startswith("InvalidInput"), msg


def test_empty_calls_and_call_level_errors(ctx, mat):
    lib = kzg.load_library()
    one = (C.c_uint64 * 1)(0)
    out = (C.c_bool * 4)()
    host = lambda nb, c, nc, ix, cl, pr, flags, v: lib.eth_kzg_amd_verify_data_columns(None, nb, c, nc, ix, cl, pr, flags, v, None)  # noqa: E731
    dev = lambda nb, c, nc, ix, cl, pr, flags, v: lib.eth_kzg_amd_verify_data_columns_device(None, nb, c, nc, ix, cl, pr, flags, v, None, None)  # noqa: E731
    for f in (host, dev):  # a NULL context is never reached
        for flags in (2, 3, 1 << 31):
            _invalid(f(0, None, 0, None, None, None, flags, None))  # a stray flag bit, also in an empty call
            _invalid(f(1, one, 1, one, one, one, flags, out))
        for flags in (0, LEAF):
            _invalid(f(1, one, (1 << 24) + 1, one, one, one, flags, out))  # an oversized count
            for missing in (1, 3, 4, 5, 7):  # a NULL array with a non-zero count
                args = [1, one, 1, one, one, one, flags, out]
                args[missing] = None
                _invalid(f(*args))
    for flags in (0, LEAF):  # n_columns = 0 is Ok, whatever else
        assert lib.eth_kzg_amd_verify_data_columns(ctx.handle, 5, None, 0, None, None, None, flags, None, None).status == 0
        assert lib.eth_kzg_amd_verify_data_columns_device(ctx.handle, 5, None, 0, None, None, None, flags, None, None, None).status == 0
    for leaf in (False, True):
        assert ctx.verify_data_columns(mat.commitments[:2], [], [], [], leaf_transcript=leaf) == ([], [])
        # n_blobs = 0: every column verifies whatever its index (an empty problem is validated without an index being read)
        assert ctx.verify_data_columns([], [0, 500, 127], [[], [], []], [[], [], []], leaf_transcript=leaf) == ([True] * 3, [0] * 3)
        assert ctx.verify_data_columns_device(0, 0, [0, 500, 127], 0, 0, leaf_transcript=leaf) == ([True] * 3, [0] * 3)
        # more blobs than a problem may hold: every column is status 3 and nothing is read (the addresses here hold nothing)
        import torch
        some = torch.zeros(64, dtype=torch.uint8, device="cuda").data_ptr()
        assert ctx.verify_data_columns_device(1 << 24, some, [0, 1], some, some, leaf_transcript=leaf) == ([False] * 2, [3] * 2)
        with pytest.raises(kzg.KzgError, match="InvalidInput"):  # a NULL array with a non-zero count, whatever the count
            ctx.verify_data_columns_device(1 << 24, some, [0, 1], 0, some, leaf_transcript=leaf)
        assert ctx.verify_cell_kzg_proof_batch_many([([], [], [], [])] * 3, leaf_transcript=leaf) == ([True] * 3, [0] * 3)
    assert lib.eth_kzg_amd_abi_version() == 6


def test_the_hook_serves_one_pass_and_refuses_missing_buffers(ctx, cases):
    lib = kzg.load_library()
    out = C.create_string_buffer(96)
    one = (C.c_uint64 * 2)(0, 1)
    i32 = (C.c_int32 * 4)()
    tail = [i32, i32, i32, out, (C.c_uint32 * 4)(), out, None, None, 0, one, out, None, one]
    for missing in (0, 1, 2, 3, 4, 5, 9, 10, 12):
        t = [None if i == missing else a for i, a in enumerate(tail)]
        assert lib.eth_kzg_amd_test_verify_data_columns_sums(None, 1, 0, one, 1, one, one, one, LEAF, *t) == 3, missing
    assert lib.eth_kzg_amd_test_verify_data_columns_sums(None, 1, 0, one, 1, one, one, one, 2, *tail) == 3  # an unknown flag
    assert lib.eth_kzg_amd_test_verify_data_columns_sums(None, 1, 2, one, 1, one, one, one, 0, *tail) == 3  # neither host nor device
    assert lib.eth_kzg_amd_test_verify_data_columns_sums(None, 1, 0, None, 1, one, one, one, 0, *tail) == 3  # blobs and no commitments
    call = cases["128x3"][0]
    wide = (call[0], call[1] * 64, call[2] * 64, call[3] * 64)  # 192 columns x 128 blobs: the call would be cut into parts
    rc, _ = column_sums(ctx, wide, "host", LEAF)
    assert rc == 3


def test_refused_columns_cost_a_status_word(ctx, mat, cases):
    """2^20 columns of 64 different blobs of which only the first two carry an index below 128: the refused ones are taken out of the
    call before its passes, so they are neither read (the device arrays here end behind column 1) nor given weights, products or arena
    (2^20 x 64 of each would not fit), and the call says what _many_ex says of the expanded input: 3 for each of them"""
    n_columns = 1 << 20
    call = _block(mat, list(range(64)), [127, 5])
    d = Dev(call)
    indices = np.full(n_columns, 128, dtype=np.uint64)
    indices[:2] = call[1]
    indices[7] = 1 << 40
    for leaf in (True, False):
        ver, st = ctx.verify_data_columns_device(64, d.ptrs[0], indices, d.ptrs[1], d.ptrs[2], leaf_transcript=leaf)
        assert ver[:2] == [True, True] and st[:2] == [0, 0] and not any(ver[2:]) and set(st[2:]) == {3}, leaf
    # refused columns BETWEEN valid ones, host and device form, against the expanded input
    mixed = _block(mat, [0, 1, 2], [3, 128, 4, 1 << 33, 5, 6, 7, 200])
    mixed[3][4] = _swap(mixed[3][4], 0, 1)
    _both(ctx, mixed, ([True, False, True, False, False, True, True, False], [0, 3, 0, 3, 0, 0, 0, 3]))
    rc, _ = column_sums(ctx, mixed, "host", LEAF)
    assert rc == 3  # the hook's outputs are indexed by column: it serves calls whose columns all pass validation


# ---- cuts: parts and chunks ---------------------------------------------------------------------------------------------------------------------
def test_200_columns_of_2_blobs(ctx, mat):
    """crosses VM_SPLIT_MIN_PROBLEMS (192); indices repeat beyond 128; one wrong column in the last third"""
    nc, wrong = 200, 171
    call = _block(mat, [0, 1], [j % 128 for j in range(nc)])
    call[3][wrong] = _swap(call[3][wrong], 0, 1)
    want = ([j != wrong for j in range(nc)], [0] * nc)
    for leaf in (False, True):
        assert ctx.verify_data_columns(*call, leaf_transcript=leaf) == want, leaf
    assert Dev(call).run(ctx, True) == want
    assert ctx.verify_cell_kzg_proof_batch_many(D.expand(*call), leaf_transcript=True) == want


def _tiled_on_device(mat, n_columns, n_blobs, wrong):
    """n_columns x n_blobs filled on the device from copies of ONE blob's cells and proofs (all blobs equal: n_u = 1), column j at index
    j % 128; column `wrong` carries the proofs of the next index -> (d_commitments, indices, d_cells, d_proofs) tensors"""
    import torch
    cells = torch.frombuffer(bytearray(b"".join(mat.cells[0])), dtype=torch.uint8).cuda().view(128, 2048)
    proofs = torch.frombuffer(bytearray(b"".join(mat.proofs[0])), dtype=torch.uint8).cuda().view(128, 48)
    idx = torch.arange(n_columns, device="cuda") % 128
    pidx = idx.clone()
    pidx[wrong] = (pidx[wrong] + 1) % 128
    d_cells = cells[idx].repeat_interleave(n_blobs, dim=0).contiguous()
    d_proofs = proofs[pidx].repeat_interleave(n_blobs, dim=0).contiguous()
    d_comm = torch.frombuffer(bytearray(mat.commitments[0] * n_blobs), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert d_cells.numel() == n_columns * n_blobs * 2048 and d_proofs.numel() == n_columns * n_blobs * 48
    return d_comm, [j % 128 for j in range(n_columns)], d_cells, d_proofs


@pytest.mark.parametrize("n_columns,what", [(192, "three concurrent parts: 192 columns and 24576 cells"), (1025, "131200 cells: more than one pass may hold")])
def test_device_resident_calls_that_are_cut(ctx, mat, n_columns, what):
    wrong = n_columns - 20
    d_comm, indices, d_cells, d_proofs = _tiled_on_device(mat, n_columns, 128, wrong)
    assert n_columns >= 192 and n_columns * 128 >= 24576 and (n_columns < 1025 or n_columns * 128 > 131072), what
    got = ctx.verify_data_columns_device(128, d_comm.data_ptr(), indices, d_cells.data_ptr(), d_proofs.data_ptr(), leaf_transcript=True)
    assert got == ([j != wrong for j in range(n_columns)], [0] * n_columns), what


def test_a_second_chunk_on_one_slot(ctx, mat):
    """fewer than 192 columns (no parts) with more than 131072 cells: 130 columns of 1025 equal blobs -- the chunk loop runs twice on one
    slot, cut at a column boundary (127 columns, then 3), the wrong column in the second chunk"""
    n_columns, n_blobs, wrong = 130, 1025, 128
    assert 127 * n_blobs <= 131072 < 128 * n_blobs
    d_comm, indices, d_cells, d_proofs = _tiled_on_device(mat, n_columns, n_blobs, wrong)
    got = ctx.verify_data_columns_device(n_blobs, d_comm.data_ptr(), indices, d_cells.data_ptr(), d_proofs.data_ptr(), leaf_transcript=True)
    assert got == ([j != wrong for j in range(n_columns)], [0] * n_columns)


# ---- device form, device list, threads ----------------------------------------------------------------------------------------------------------
def test_odd_addresses_behind_work_on_the_callers_stream(ctx, cases):
    import torch
    call, wrong, _, _ = cases["two-proofs-swapped"]
    want = ([j not in wrong for j in range(len(call[1]))], [0] * len(call[1]))
    stream = torch.cuda.Stream()
    for leaf in (True, False):
        d = Dev(call, shift=1, stream=stream)
        assert all(p % 2 == 1 for p in d.ptrs)
        assert d.run(ctx, leaf, stream=stream.cuda_stream) == want, leaf
    stream.synchronize()


def test_device_list_and_foreign_memory(ctx, cases):
    """the device list 0,0; host memory in the place of each device pointer.  Memory of ANOTHER device is tried only where the machine has
    a second GPU: on a one-GPU machine that case does not run (the owner look-up it would reach is the one the host-memory case reaches)"""
    call, wrong, _, _ = cases["two-equal-among-different"]
    nc = len(call[1])
    want = ([j not in wrong for j in range(nc)], [0] * nc)
    multi = _ctx(devices=[0, 0], ETH_KZG_AMD_HOST_THREADS=str(HOST_THREADS))
    try:
        d = Dev(call)
        for leaf in (True, False):
            assert multi.verify_data_columns(*call, leaf_transcript=leaf) == want  # the host form cut by column over the list
            assert d.run(multi, leaf) == want                                      # the device form on the owner of the buffers
        host = np.zeros(len(call[0]) * nc * 2048, dtype=np.uint8)
        for c in (multi, ctx):  # all three pointers are resolved: host memory in any place is InvalidInput, never dereferenced
            for k in range(3):
                ptrs = list(d.ptrs)
                ptrs[k] = host.ctypes.data
                for leaf in (True, False):
                    with pytest.raises(kzg.KzgError, match="InvalidInput"):
                        c.verify_data_columns_device(d.n_blobs, ptrs[0], d.indices, ptrs[1], ptrs[2], leaf_transcript=leaf)
        import torch
        if torch.cuda.device_count() > 1:  # memory of a device the context does not list
            with torch.cuda.device(1):
                other = Dev(call)
            with pytest.raises(kzg.KzgError, match="InvalidInput"):
                other.run(ctx, True)
        assert d.run(multi, True) == want  # and the context goes on working
    finally:
        multi.close()


def test_four_threads_on_one_context(ctx, cases):
    call, wrong, _, _ = cases["two-proofs-swapped"]
    nc = len(call[1])
    calls = []
    for t in range(4):  # the columns rotated: every thread expects its own verdicts
        rot = lambda x: x[t:] + x[:t]  # noqa: E731
        calls.append(((call[0], rot(call[1]), rot(call[2]), rot(call[3])), ([((j + t) % nc) not in wrong for j in range(nc)], [0] * nc)))
    assert len({tuple(w[0]) for _, w in calls}) == 4
    errors = []

    def run(t):
        try:
            for _ in range(3):
                assert ctx.verify_data_columns(*calls[t][0], leaf_transcript=True) == calls[t][1], t
                assert Dev(calls[t][0]).run(ctx, True) == calls[t][1], t
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    th = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


# ---- the reference's vectors --------------------------------------------------------------------------------------------------------------------
def test_the_seven_valid_prover_vectors_as_one_block(ctx):
    golden = sorted((k, c) for k, c in vectors.load("compute_cells_and_kzg_proofs").items() if c["output"] is not None)
    assert len(golden) == 7
    commitments = [ctx.blob_to_kzg_commitment(c["input"]["blob"]) for _, c in golden]
    indices = list(range(128))
    cells = [[c["output"][0][j] for _, c in golden] for j in indices]
    proofs = [[c["output"][1][j] for _, c in golden] for j in indices]
    for leaf in (False, True):
        assert ctx.verify_data_columns(commitments, indices, cells, proofs, leaf_transcript=leaf) == ([True] * 128, [0] * 128), leaf
    assert Dev((commitments, indices, cells, proofs)).run(ctx, True) == ([True] * 128, [0] * 128)
