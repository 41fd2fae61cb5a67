"""Partial data columns, a bitmap of the blobs present per column: eth_kzg_amd_verify_partial_data_columns / _device.

Column j of a call is the problem tests/partial_columns.py expands it into, so every check here is against the EXPANDED input: verdicts
from the CPU oracle, verdicts and statuses from eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex, and -- through the hook
eth_kzg_amd_test_verify_partial_data_columns_sums, a tap on the pass's own read-backs -- every leaf, digest, per-column pair, weight,
folded pair and probe byte for byte against the tap of the expanded pass (eth_kzg_amd_test_verify_many_sums_ex, which
tests/test_gpu_many_leaf.py and tests/test_verify_inputs.py hold to the statement in hashlib and Python integers).  The tap's counts tell
the sparse pair list from the dense addressing: n + P + Bc scalar multiplications for the P (column, commitment) pairs that hold a
cell, where the dense column pass launches n + Bc n_u + Bc.
The context is test_verify_inputs.py's many_ctx: small tables, two host threads -- the short-chain form up to 4 columns, the fold above.
Material: three golden blobs of the reference's prover vectors and 127 seeded blobs, their cells and proofs from the library's prover."""
import ctypes as C
import threading

import numpy as np
import pytest

import data_columns as D
import partial_columns as P
import small_order as S
import synth
import test_gpu_data_columns as G
import vectors
import verify_transcript as T

kzg = G.kzg
pytestmark = pytest.mark.gpu

LEAF = G.LEAF
HOST_THREADS = T.MANY_HOST_THREADS
N_GOLDEN, N_BLOBS = 3, 130
INF = T.INF
_expanded = {}  # the expanded pass's tap and the oracle's verdicts, computed once per case, shared by the ways, never changed


@pytest.fixture(scope="module")
def ctx():
    c = G._ctx(ETH_KZG_AMD_HOST_THREADS=str(HOST_THREADS))
    yield c
    c.close()


@pytest.fixture(scope="module")
def mat(ctx):
    golden = sorted((k, c) for k, c in vectors.load("compute_cells_and_kzg_proofs").items() if c["output"] is not None)[:N_GOLDEN]
    seeded = [synth.seeded_blob(8100 + i) for i in range(N_BLOBS - N_GOLDEN)]
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(seeded)
    assert st == [0] * len(seeded)
    m = G.Mat()
    m.cells = [c["output"][0] for _, c in golden] + cells
    m.proofs = [c["output"][1] for _, c in golden] + proofs
    m.commitments = [ctx.blob_to_kzg_commitment(b) for b in [c["input"]["blob"] for _, c in golden] + seeded]
    assert len(set(m.commitments)) == N_BLOBS and INF not in m.commitments
    return m


def _partial(mat, picks, indices, present):
    return P.mask(D.block(mat.commitments, mat.cells, mat.proofs, picks, indices), present)


class Dev:
    """the three packed byte arrays of a partial call in device memory, `shift` bytes into their allocations"""

    def __init__(self, call, shift=0, stream=None):
        import torch
        self.n_blobs, self.indices, self.present = len(call[0]), call[1], call[2]
        self.keep, self.ptrs = [], []
        for raw in P.flat_bytes(call):
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
        return ctx.verify_partial_data_columns_device(self.n_blobs, self.ptrs[0], self.indices, self.present, self.ptrs[1], self.ptrs[2],
                                                      stream=stream, leaf_transcript=leaf)


def partial_sums(ctx, call, where, flags, max_probes=64):
    """eth_kzg_amd_test_verify_partial_data_columns_sums -> (return code, Sums with .counts = (commitments decoded, multiplications))"""
    lib = kzg.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nb, nc = len(call[0]), len(call[1])
    n_cells = sum(len(c) for c in call[3])
    ver, st, form, sums, rho, fold, pr, ps, npr, dig, leaves = bufs = G._buffers(nc, n_cells, max_probes)
    counts = (C.c_uint64 * 2)()
    tail = (flags, ver, st, form, sums, rho, fold, pr, ps, max_probes, C.byref(npr), dig, leaves, counts)
    if where == "host":
        _, _, ca, idx, ba, cla, pa, _keep = ctx._marshal_partial_columns(*call)
        rc = lib.eth_kzg_amd_test_verify_partial_data_columns_sums(ctx.handle, nb, 0, vp(ca), nc, vp(idx), vp(ba), vp(cla), vp(pa), *tail)
    else:
        d = Dev(call)
        idx = np.array(call[1], dtype=np.uint64)
        bits, _ = ctx._present_words(nb, call[2])
        rc = lib.eth_kzg_amd_test_verify_partial_data_columns_sums(ctx.handle, nb, 1, C.c_void_p(d.ptrs[0]), nc, vp(idx), vp(bits),
                                                                   C.c_void_p(d.ptrs[1]), C.c_void_p(d.ptrs[2]), *tail)
    out = G._unpack(nc, n_cells, *bufs, max_probes)
    out.counts = (counts[0], counts[1])
    return rc, out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
def _cases(mat):
    """name -> (partial call, wrong columns, form (small, folded, searched), the dense call where every bit is set)"""
    out = {}

    def add(name, picks, indices, present, wrong=(), change=None, form=None):
        dense = D.block(mat.commitments, mat.cells, mat.proofs, picks, indices)
        call = P.mask(dense, present)
        if change:
            change(call)
        full = all(p == (1 << len(picks)) - 1 for p in present) and not change
        out[name] = (call, set(wrong), form, dense if full else None)

    short, folded, searched = (True, False, False), (False, True, False), (False, True, True)
    six = list(range(6))
    # 3 columns x 6 blobs at the edge values of h^64: index 0 (h^64 = 1), 64 (brp7 = 1) and 127
    add("3x6-every-bit", six, [0, 64, 127], [0b111111] * 3, form=short)
    add("3x6-blob-0-only", six, [0, 64, 127], [0b000001] * 3, form=short)
    add("3x6-every-second", six, [0, 64, 127], [0b101010] * 3, form=short)
    add("3x6-three-masks", six, [127, 0, 64], [0b111111, 0b000001, 0b101010], form=short)
    # repeated commitments: the column's own list and re-ranked rows (flags = 0 hashes them) against the pass-wide rows the kernels read
    add("blob-0-is-blob-2-and-only-2-3-present", [0, 1, 0, 2], [3, 4, 5], [0b1100] * 3, form=short)
    add("own-list-in-another-order-than-the-calls", [0, 1, 0], [3, 4], [0b110, 0b011], form=short)
    add("one-index-twice-disjoint-masks", six, [5, 5], [0b000111, 0b111000], form=short)
    add("empty-column-between-full-ones", six, [1, 500, 2], [0b111111, 0, 0b111111], form=short)
    add("70-blobs-bits-63-64-69", list(range(70)), [9, 10, 11], [1 << 63 | 1 << 64 | 1 << 69, 1 << 63, 1 << 64 | 1 << 69], form=short)
    add("129x130-one-cell-each", list(range(130)), [j % 128 for j in range(129)], [1 << j for j in range(129)], form=folded)
    add("2x6-search", [0, 1], [0, 1, 64, 127, 3, 2], [0b11, 0b01, 0b10, 0b11, 0b11, 0b10], wrong=[4],
        change=lambda c: c[4][4].__setitem__(1, G._negated(c[4][4][1])), form=searched)
    add("cells-of-two-present-blobs-swapped", six, [0, 64, 127], [0b101010] * 3, wrong=[1],
        change=lambda c: c[3].__setitem__(1, G._swap(c[3][1], 0, 2)), form=short)
    add("5-unequal-columns-folded", list(range(9)), [127, 1, 0, 64, 9], [0b1, 0b111111111, 0b10101, 0b100000000, 0b11110000], form=folded)
    return out


CASE_NAMES = ["3x6-every-bit", "3x6-blob-0-only", "3x6-every-second", "3x6-three-masks", "blob-0-is-blob-2-and-only-2-3-present",
              "own-list-in-another-order-than-the-calls", "one-index-twice-disjoint-masks", "empty-column-between-full-ones",
              "70-blobs-bits-63-64-69", "129x130-one-cell-each", "2x6-search", "cells-of-two-present-blobs-swapped", "5-unequal-columns-folded"]


@pytest.fixture(scope="module")
def cases(mat):
    c = _cases(mat)
    assert list(c) == CASE_NAMES
    return c


def _reference(ctx, oracle, name, call, flags):
    """the expanded pass: its tap on this build, and the oracle's verdicts"""
    key = (name, flags)
    if key not in _expanded:
        problems = P.expand(*call)
        assert None not in problems
        rc, tap = G.expanded_sums(ctx, problems, flags)
        assert rc == 0
        if name not in _expanded:
            _expanded[name] = [oracle.verify_cell_kzg_proof_batch(*p) for p in problems]
        _expanded[key] = (problems, tap, _expanded[name])
    return _expanded[key]


WAYS = {"host": ("host", 0), "host-leaf": ("host", LEAF), "device": ("device", 0), "device-leaf": ("device", LEAF)}


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_a_partial_pass_equals_the_expanded_pass_byte_for_byte(ctx, oracle, cases, name, way):
    where, flags = WAYS[way]
    call, wrong, form, dense = cases[name]
    nc = len(call[1])
    problems, ref, verdicts = _reference(ctx, oracle, name, call, flags)
    n_cells = sum(len(p[1]) for p in problems)
    assert verdicts == [j not in wrong for j in range(nc)], (name, verdicts)  # the oracle names exactly the columns made wrong
    assert (ref.verified, ref.status) == (verdicts, [0] * nc), name
    rc, got = partial_sums(ctx, call, where, flags)
    assert rc == 0, (name, way, rc)
    assert (got.verified, got.status) == (verdicts, [0] * nc), (name, way, got.verified, got.status)
    assert (got.small, got.folded, got.searched) == (ref.small, ref.folded, ref.searched) == form, (name, way, got.small, got.folded, got.searched)
    assert got.digests == ref.digests, (name, way, [j for j in range(nc) if got.digests[j] != ref.digests[j]])
    bad = [(j, got.sums[j][:48] == ref.sums[j][:48], got.sums[j][48:] == ref.sums[j][48:]) for j in range(nc) if got.sums[j] != ref.sums[j]]
    assert not bad, "%s %s: (column, A equal, B equal) %s" % (name, way, bad)
    assert all(s[0] != 0xff for s, p in zip(got.sums, problems) if p[1])  # no slot of a column with cells still holds its poison
    assert got.fold == ref.fold and got.fold_verdict == ref.fold_verdict, (name, way)
    if got.folded:  # (a pass that is not folded computes no weights)
        assert got.rho == ref.rho, (name, way)
    assert got.n_probes == ref.n_probes and got.probes == ref.probes, (name, way)
    if flags:
        assert got.leaves == ref.leaves, (name, way, [k for k in range(n_cells) if got.leaves[k] != ref.leaves[k]][:10])
    # the sparse pair list: the call's unique commitments once, n + P + Bc products
    assert got.counts == P.counts(call[0], call[1], call[2]), (name, way, got.counts)
    if dense is not None:  # every bit set: the dense hook's output, counts included
        rc, full = G.column_sums(ctx, dense, where, flags)
        assert rc == 0
        assert (full.verified, full.status, full.digests, full.sums, full.fold, full.probes, full.counts) == \
               (got.verified, got.status, got.digests, got.sums, got.fold, got.probes, got.counts), (name, way)
        if flags:
            assert full.leaves == got.leaves


# ---- the public calls -------------------------------------------------------------------------------------------------------------------------
def _both(ctx, call, want):
    """the expanded call, the host form and the device form, under both flag values; a column refused at validation has no expanded
    problem (tests/partial_columns.py: expand) and must come out (False, 3)"""
    problems = P.expand(*call)
    kept = [p for p in problems if p is not None]
    d = Dev(call)
    for leaf in (False, True):
        ver, st = ctx.verify_cell_kzg_proof_batch_many(kept, leaf_transcript=leaf)
        ver, st = iter(ver), iter(st)
        merged = ([False if p is None else next(ver) for p in problems], [3 if p is None else next(st) for p in problems])
        assert merged == want, ("expanded", leaf, merged)
        assert ctx.verify_partial_data_columns(*call, leaf_transcript=leaf) == want, ("host", leaf)
        assert d.run(ctx, leaf) == want, ("device", leaf)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_public_calls_agree_with_many_ex_on_the_expanded_input(ctx, cases, name):
    call, wrong, _, _ = cases[name]
    nc = len(call[1])
    _both(ctx, call, ([j not in wrong for j in range(nc)], [0] * nc))


def test_statuses_in_the_reference_order(ctx, mat):
    r_be = T.R.to_bytes(32, "big")
    six = list(range(6))
    # a stray bit: 3 for that column only, its entries in the packed arrays skipped unread
    call = _partial(mat, six, [0, 1, 2], [0b111, 0b1000011, 0b110000])
    _both(ctx, call, ([True, False, True], [0, 3, 0]))
    # an index >= 128: 3 where the column holds a cell, an empty problem where it holds none
    call = _partial(mat, six, [128, 1 << 40, 200, 127], [0b1, 0, 0b11, 0b100001])
    _both(ctx, call, ([False, True, False, True], [3, 0, 3, 0]))
    # a bad commitment marks the columns that hold a cell of that blob and no others; then proofs (2), then cells (1)
    call = _partial(mat, six, [0, 64, 127, 5, 6], [0b000110, 0b111001, 0b001001, 0b010001, 0b100100])
    call[0][1] = T.off_subgroup_point()                       # blob 1: column 0 only
    call[4][2][1] = T.off_subgroup_point()                    # column 2: a bad proof
    call[3][3][0] = call[3][3][0][:-32] + r_be                # column 3: a non-canonical cell
    call[4][4][0] = T.off_subgroup_point()                    # column 4: a bad proof AND a bad cell: the proof is reported
    call[3][4][1] = r_be + call[3][4][1][32:]
    _both(ctx, call, ([False, True, False, False, False], [2, 0, 2, 1, 2]))
    # a bad commitment of a present blob AND a non-canonical cell in one column: the commitment is reported
    call = _partial(mat, six, [7, 8], [0b11, 0b01])
    call[0][1] = T.off_subgroup_point()
    call[3][0][0] = r_be + call[3][0][0][32:]
    _both(ctx, call, ([False, True], [2, 0]))


def test_small_order_points_as_commitment_and_as_proof(ctx, mat):
    six = list(range(6))
    for l, pt in S.small_order_points().items():
        enc = S.encode(pt)
        absent = _partial(mat, six, [0, 1], [0b001111, 0b101100])
        absent[0][4] = enc  # the commitment of a blob that no column holds: no effect
        _both(ctx, absent, ([True, True], [0, 0]))
        present = _partial(mat, six, [0, 1], [0b011111, 0b101100])
        present[0][4] = enc  # a blob present in column 0 only: column 0 gets 2, column 1 its verdict
        present[4][1] = G._swap(present[4][1], 0, 1)
        _both(ctx, present, ([False, False], [2, 0]))
        as_proof = _partial(mat, six, [0, 1, 2], [0b11, 0b110, 0b1])
        as_proof[4][1][1] = enc
        _both(ctx, as_proof, ([True, False, True], [0, 2, 0]))


def test_empty_calls_and_call_level_errors(ctx, mat):
    lib = kzg.load_library()
    one = (C.c_uint64 * 1)(0)
    out = (C.c_bool * 4)()
    host = lambda nb, c, nc, ix, pm, cl, pr, flags, v: lib.eth_kzg_amd_verify_partial_data_columns(None, nb, c, nc, ix, pm, cl, pr, flags, v, None)  # noqa: E731
    dev = lambda nb, c, nc, ix, pm, cl, pr, flags, v: lib.eth_kzg_amd_verify_partial_data_columns_device(None, nb, c, nc, ix, pm, cl, pr, flags, v, None, None)  # noqa: E731
    for f in (host, dev):  # a NULL context is never reached
        for flags in (2, 3, 1 << 31):
            G._invalid(f(0, None, 0, None, None, None, None, flags, None))  # a stray flag bit, also in an empty call
            G._invalid(f(1, one, 1, one, one, one, one, flags, out))
        for flags in (0, LEAF):
            G._invalid(f(1, one, (1 << 24) + 1, one, one, one, one, flags, out))  # an oversized count
            for missing in (1, 3, 4, 5, 6, 8):  # a NULL array with a non-zero count: commitments, indices, present, cells, proofs, verified
                args = [1, one, 1, one, one, one, one, flags, out]
                args[missing] = None
                G._invalid(f(*args))
            for missing in (3, 8):  # without blobs: indices and verdicts still
                args = [0, None, 1, one, None, None, None, flags, out]
                args[missing] = None
                G._invalid(f(*args))
    for flags in (0, LEAF):  # n_columns = 0 is Ok, whatever else
        assert lib.eth_kzg_amd_verify_partial_data_columns(ctx.handle, 5, None, 0, None, None, None, None, flags, None, None).status == 0
        assert lib.eth_kzg_amd_verify_partial_data_columns_device(ctx.handle, 5, None, 0, None, None, None, None, flags, None, None, None).status == 0
    import torch
    some = torch.zeros(64, dtype=torch.uint8, device="cuda").data_ptr()
    for leaf in (False, True):
        assert ctx.verify_partial_data_columns(mat.commitments[:2], [], [], [], [], leaf_transcript=leaf) == ([], [])
        # n_blobs = 0 (no bitmap words at all) and columns without a bit: every column verifies whatever its index
        assert ctx.verify_partial_data_columns([], [0, 500, 127], [0, 0, 0], [[], [], []], [[], [], []], leaf_transcript=leaf) == ([True] * 3, [0] * 3)
        assert ctx.verify_partial_data_columns_device(0, 0, [0, 500, 127], [0, 0, 0], 0, 0, leaf_transcript=leaf) == ([True] * 3, [0] * 3)
        assert ctx.verify_partial_data_columns(mat.commitments[:2], [0, 500], [0, 0], [[], []], [[], []], leaf_transcript=leaf) == ([True] * 2, [0] * 2)
        assert ctx.verify_partial_data_columns_device(2, some, [0, 500], [0, 0], some, some, leaf_transcript=leaf) == ([True] * 2, [0] * 2)
        # only refused columns: nothing is read (the addresses here hold nothing of the kind)
        assert ctx.verify_partial_data_columns_device(2, some, [0, 128], [0b100, 0b01], some, some, leaf_transcript=leaf) == ([False] * 2, [3] * 2)
    # more blobs than a problem may hold: every column is status 3 and nothing is read, the bitmaps included
    big = (C.c_uint64 * 2)(0, 1)
    ver, st = (C.c_bool * 2)(True, True), (C.c_int32 * 2)()
    res = lib.eth_kzg_amd_verify_partial_data_columns_device(ctx.handle, 1 << 24, C.c_void_p(some), 2, big, C.c_void_p(some), C.c_void_p(some),
                                                             C.c_void_p(some), LEAF, ver, st, None)
    assert res.status == 0 and list(ver) == [False, False] and list(st) == [3, 3]
    assert lib.eth_kzg_amd_abi_version() == 6


def test_the_hook_serves_one_pass_of_accepted_columns(ctx, mat):
    six = list(range(6))
    rc, _ = partial_sums(ctx, _partial(mat, six, [0, 1], [0b11, 0b1000001]), "host", LEAF)
    assert rc == 3  # the hook's outputs are indexed by column: it serves calls whose columns all pass validation
    wide = _partial(mat, list(range(128)), [j % 128 for j in range(192)], [(1 << 128) - 1] * 192)  # 192 columns, 24576 cells: cut into parts
    rc, _ = partial_sums(ctx, wide, "host", LEAF)
    assert rc == 3


# ---- device form, device list, threads, cuts ------------------------------------------------------------------------------------------------------
def test_packed_arrays_at_odd_addresses_behind_work_on_the_callers_stream(ctx, cases):
    import torch
    call, wrong, _, _ = cases["2x6-search"]
    want = ([j not in wrong for j in range(len(call[1]))], [0] * len(call[1]))
    stream = torch.cuda.Stream()
    for leaf in (True, False):
        d = Dev(call, shift=1, stream=stream)
        assert all(p % 2 == 1 for p in d.ptrs)
        assert d.run(ctx, leaf, stream=stream.cuda_stream) == want, leaf
    stream.synchronize()


def test_device_list_and_foreign_memory(ctx, cases):
    """the device list 0,0 (the host form cut by column, unequal columns and a refused one among them); host memory in the place of each
    device pointer"""
    call, wrong, _, _ = cases["5-unequal-columns-folded"]
    call = (call[0], call[1] + [3], call[2] + [1 << 9], call[3] + [[]], call[4] + [[]])  # a stray bit in the last column
    nc = len(call[1])
    want = ([True] * (nc - 1) + [False], [0] * (nc - 1) + [3])
    multi = G._ctx(devices=[0, 0], ETH_KZG_AMD_HOST_THREADS=str(HOST_THREADS))
    try:
        d = Dev(call)
        for leaf in (True, False):
            assert multi.verify_partial_data_columns(*call, leaf_transcript=leaf) == want
            assert d.run(multi, leaf) == want
        host = np.zeros(1 << 20, dtype=np.uint8)
        for c in (multi, ctx):  # all three pointers are resolved: host memory in any place is InvalidInput, never dereferenced
            for k in range(3):
                ptrs = list(d.ptrs)
                ptrs[k] = host.ctypes.data
                for leaf in (True, False):
                    with pytest.raises(kzg.KzgError, match="InvalidInput"):
                        c.verify_partial_data_columns_device(d.n_blobs, ptrs[0], d.indices, d.present, ptrs[1], ptrs[2], leaf_transcript=leaf)
        assert d.run(multi, True) == want  # and the context goes on working
    finally:
        multi.close()


def test_four_threads_on_one_context(ctx, cases):
    call, wrong, _, _ = cases["2x6-search"]
    nc = len(call[1])
    calls = []
    for t in range(4):  # the columns rotated: every thread expects its own verdicts
        rot = lambda x: x[t:] + x[:t]  # noqa: E731
        calls.append(((call[0], rot(call[1]), rot(call[2]), rot(call[3]), rot(call[4])), ([((j + t) % nc) not in wrong for j in range(nc)], [0] * nc)))
    assert len({tuple(w[0]) for _, w in calls}) == 4
    errors = []

    def run(t):
        try:
            for _ in range(3):
                assert ctx.verify_partial_data_columns(*calls[t][0], leaf_transcript=True) == calls[t][1], t
                assert Dev(calls[t][0]).run(ctx, True) == calls[t][1], t
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    th = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


def test_a_device_resident_call_that_is_cut(ctx, mat):
    """1025 columns over 128 blobs, popcounts cycling 1..128 (column j holds blobs 0 .. j % 128 under index j % 128): 66049 cells in
    three concurrent parts of unequal columns, filled on the device, two columns wrong; against _many_device_ex on the expanded input"""
    import torch
    n_columns, nb, wrong = 1025, 128, (300, 1001)
    cells = torch.frombuffer(bytearray(b"".join(c for b in range(nb) for c in mat.cells[b])), dtype=torch.uint8).cuda().view(nb, 128, 2048)
    proofs = torch.frombuffer(bytearray(b"".join(p for b in range(nb) for p in mat.proofs[b])), dtype=torch.uint8).cuda().view(nb, 128, 48)
    indices = [j % 128 for j in range(n_columns)]
    present = [(1 << (1 + j % 128)) - 1 for j in range(n_columns)]
    blob = torch.tensor([i for j in range(n_columns) for i in range(1 + j % 128)], device="cuda")
    col = torch.tensor([j % 128 for j in range(n_columns) for _ in range(1 + j % 128)], device="cuda")
    pcol = col.clone()
    starts = [0]
    for j in range(n_columns):
        starts.append(starts[-1] + 1 + j % 128)
    for j in wrong:  # the column's last proof (of blob j % 128, a seeded one) is that of the next index
        assert j % 128 >= N_GOLDEN and mat.proofs[j % 128][j % 128] != mat.proofs[j % 128][(j + 1) % 128]
        pcol[starts[j + 1] - 1] = (pcol[starts[j + 1] - 1] + 1) % 128
    d_cells, d_proofs = cells[blob, col].contiguous(), proofs[blob, pcol].contiguous()
    comm = torch.frombuffer(bytearray(b"".join(mat.commitments[:nb])), dtype=torch.uint8).cuda().view(nb, 48)
    d_comm, d_comm_expanded, d_idx = comm.contiguous(), comm[blob].contiguous(), col.to(torch.int64).contiguous()
    torch.cuda.synchronize()
    n = starts[-1]
    assert n == 66049 >= 24576 and n_columns >= 192 and d_cells.numel() == n * 2048 and d_proofs.numel() == n * 48
    want = ([j not in wrong for j in range(n_columns)], [0] * n_columns)
    got = ctx.verify_partial_data_columns_device(nb, d_comm.data_ptr(), indices, present, d_cells.data_ptr(), d_proofs.data_ptr(), leaf_transcript=True)
    assert got == want, [(j, got[0][j], got[1][j]) for j in range(n_columns) if got[0][j] != want[0][j] or got[1][j]][:10]
    ref = ctx.verify_cell_kzg_proof_batch_many_device(starts, d_comm_expanded.data_ptr(), d_idx.data_ptr(), d_cells.data_ptr(), d_proofs.data_ptr(),
                                                      leaf_transcript=True)
    assert ref == want
