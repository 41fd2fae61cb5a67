"""A block's data columns recovered and checked against the block's commitments: eth_kzg_amd_recover_data_columns_checked, host and
device forms.

With exactly 64 columns ANY canonical bytes decode to some polynomial of degree below 4096, so the unchecked recovery answers status 0
with cells and proofs of a polynomial nobody committed to; the checked call commits to the recovered coefficients and compares the 48
bytes with the caller's (status 6).  Every check here is `==` on bytes or statuses; there are no tolerances.

The block is 70 seeded blobs (synth.seeded_blob), blob 5 replaced by the all-zero blob, built ONCE: commitments, cells and proofs come
from blob_to_kzg_commitment_device / compute_cells_and_kzg_proofs_device and are never changed; the first three blobs are also held
against the CPU oracle.  The blobs themselves are ground truth no library call produced: out_blobs must equal them.  Shapes, the
smallest that reach each path: n = 1, 3 and 64; 65, where the padded stride is 128 -- a second lane group with one live blob in the MSM,
the fold and the compress; 70 under ETH_KZG_AMD_DEVICE_BATCH_MAX=64, sub-batches 64 + 6 with r0 != 0.  Device outputs lie between 4096
guard bytes of 0xA5 on either side."""
import importlib
import os
import random

import numpy as np
import pytest

import block_columns as B
import synth

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu

N_BLOCK, GUARD, ZERO_BLOB = 70, 4096, 5
BLOB, CELL, PROOF, CELLS = 131072, 2048, 48, 128
NOT_CANONICAL = b"\xff" * 32  # >= r
IDENTITY = b"\xc0" + b"\x00" * 47
PRE = 0xC3


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
    c = _ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx64():
    c = _ctx(ETH_KZG_AMD_DEVICE_BATCH_MAX="64")
    yield c
    c.close()


class Block:
    """blob-major: host blobs, and the device tensors blobs [n][131072], comm [n][48], cells [n][128][2048], proofs [n][128][48]"""


@pytest.fixture(scope="module")
def block(ctx):
    import torch
    blk = Block()
    blk.blobs = [synth.seeded_blob(7300 + i) for i in range(N_BLOCK)]
    blk.blobs[ZERO_BLOB] = bytes(BLOB)
    blk.d_blobs = torch.from_numpy(np.frombuffer(b"".join(blk.blobs), dtype=np.uint8).copy()).cuda().view(N_BLOCK, BLOB)
    blk.comm = torch.zeros(N_BLOCK, PROOF, dtype=torch.uint8, device="cuda")
    blk.cells = torch.zeros(N_BLOCK, CELLS, CELL, dtype=torch.uint8, device="cuda")
    blk.proofs = torch.zeros(N_BLOCK, CELLS, PROOF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.blob_to_kzg_commitment_device(N_BLOCK, blk.d_blobs.data_ptr(), blk.comm.data_ptr()) == [0] * N_BLOCK
    assert ctx.compute_cells_and_kzg_proofs_device(N_BLOCK, blk.d_blobs.data_ptr(), blk.cells.data_ptr(), blk.proofs.data_ptr()) == [0] * N_BLOCK
    torch.cuda.synchronize()
    blk._host = {}
    return blk


def _host_columns(block, n):
    """(commitments[i], cells[c][i], proofs[c][i]) of the first n blobs as byte strings"""
    if n not in block._host:
        comm = block.comm[:n].cpu().numpy().tobytes()
        cells = B.unflat(block.cells[:n].cpu().numpy().tobytes(), n, CELLS, CELL)
        proofs = B.unflat(block.proofs[:n].cpu().numpy().tobytes(), n, CELLS, PROOF)
        block._host[n] = ([comm[PROOF * i:PROOF * i + PROOF] for i in range(n)], B.to_columns(cells), B.to_columns(proofs))
    return block._host[n]


def _column_sets():
    rng = random.Random("recover-checked:held")
    return {"even": list(range(0, 128, 2)), "64-127": list(range(64, 128)), "random-64": sorted(rng.sample(range(128), 64)),
            "65": sorted(rng.sample(range(128), 65)), "all": list(range(128))}


SETS = _column_sets()


class Guarded:
    """a device array of `size` bytes with GUARD bytes of 0xA5 on both sides, itself filled with `fill`"""

    def __init__(self, size, fill=0x5A):
        import torch
        self.size = size
        self.t = torch.full((size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t[GUARD:GUARD + size] = fill
        self.ptr = self.t.data_ptr() + GUARD

    def body(self):
        return self.t[GUARD:GUARD + self.size]

    def intact(self):
        return bool((self.t[:GUARD] == 0xA5).all()) and bool((self.t[GUARD + self.size:] == 0xA5).all())


class Outs:
    """the four device outputs of a checked call on n blobs; want: which of (blobs, commitments, cells, proofs) exist"""

    def __init__(self, n, want=(True, True, True, True)):
        self.n = n
        sizes = (n * BLOB, n * PROOF, CELLS * n * CELL, CELLS * n * PROOF)
        self.blobs, self.comm, self.cells, self.proofs = [Guarded(s) if w else None for s, w in zip(sizes, want)]

    def all(self):
        return [g for g in (self.blobs, self.comm, self.cells, self.proofs) if g is not None]

    def ptrs(self):
        return dict(d_out_blobs=self.blobs.ptr if self.blobs else 0, d_out_commitments=self.comm.ptr if self.comm else 0,
                    d_out_cells=self.cells.ptr if self.cells else 0, d_out_proofs=self.proofs.ptr if self.proofs else 0)

    def intact(self):
        return all(g.intact() for g in self.all())

    def untouched(self):
        return all(bool((g.body() == 0x5A).all()) for g in self.all())

    def expect(self, block, picks, skip=()):
        """every output that exists against the block's blobs `picks` (indices into the block), but for the positions in `skip`"""
        import torch
        torch.cuda.synchronize()
        assert self.intact()
        n = self.n
        keep = torch.tensor([i for i in range(n) if i not in skip], device="cuda")
        src = torch.tensor(list(picks), device="cuda")[keep]
        if self.blobs:
            assert torch.equal(self.blobs.body().view(n, BLOB)[keep], block.d_blobs[src])
        if self.comm:
            assert torch.equal(self.comm.body().view(n, PROOF)[keep], block.comm[src])
        if self.cells:
            assert torch.equal(self.cells.body().view(CELLS, n, CELL)[:, keep], block.cells[src].permute(1, 0, 2))
        if self.proofs:
            assert torch.equal(self.proofs.body().view(CELLS, n, PROOF)[:, keep], block.proofs[src].permute(1, 0, 2))


def _device_input(given):
    import torch
    return torch.from_numpy(np.frombuffer(B.flat(given), dtype=np.uint8).copy()).cuda()


def _device_bytes(items):
    import torch
    return torch.from_numpy(np.frombuffer(b"".join(items), dtype=np.uint8).copy()).cuda()


def _expect_host(block, n, got, skip=(), want=(True, True, True, True)):
    """a host call's (blobs, commitments, cells, proofs) against the block: exact, None where not asked for, prefill at `skip`"""
    comm, cells, proofs = _host_columns(block, n)
    g_blobs, g_comm, g_cells, g_proofs = got
    for g, w in zip(got, want):
        assert (g is not None) == w
    for i in range(n):
        bad = i in skip
        if g_blobs is not None:
            assert g_blobs[i] == (bytes([PRE]) * BLOB if bad else block.blobs[i])
        if g_comm is not None:
            assert g_comm[i] == (bytes([PRE]) * PROOF if bad else comm[i])
        if g_cells is not None:
            assert all(g_cells[c][i] == (bytes([PRE]) * CELL if bad else cells[c][i]) for c in range(CELLS))
        if g_proofs is not None:
            assert all(g_proofs[c][i] == (bytes([PRE]) * PROOF if bad else proofs[c][i]) for c in range(CELLS))


# ---- the fixture itself -----------------------------------------------------------------------------------------------------------
def test_the_block_equals_the_oracle_on_its_first_blobs(ctx, block):
    from oracle_lib import Oracle
    oracle = Oracle(use_precomp=True, threads=min(8, os.cpu_count() or 1))
    try:
        comm, cells, proofs = _host_columns(block, 3)
        for i in range(3):
            oc, op = oracle.compute_cells_and_kzg_proofs(block.blobs[i])
            assert [cells[c][i] for c in range(CELLS)] == oc and [proofs[c][i] for c in range(CELLS)] == op
            assert comm[i] == oracle.blob_to_kzg_commitment(block.blobs[i])
    finally:
        oracle.close()
    assert _host_columns(block, 6)[0][ZERO_BLOB] == IDENTITY  # the zero blob's commitment is the identity


# ---- right input -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("n", [1, 3, 65])
def test_right_input_host_form(ctx, block, n, name):
    comm, cells, proofs = _host_columns(block, n)
    given = B.cut_columns(cells, SETS[name])
    st, *got = ctx.recover_data_columns_checked(SETS[name], given, comm, prefill=PRE)
    assert st == [0] * n
    _expect_host(block, n, got)
    plain = ctx.recover_data_columns(SETS[name], given)
    assert (st, got[2], got[3]) == plain  # the unchecked call's statuses and bytes
    if n > ZERO_BLOB:
        assert got[1][ZERO_BLOB] == IDENTITY and got[0][ZERO_BLOB] == bytes(BLOB)


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("n", [1, 3, 64, 65])
def test_right_input_device_form(ctx, block, n, name):
    import torch
    held = torch.tensor(SETS[name], device="cuda")
    d_in = block.cells[:n].permute(1, 0, 2)[held].contiguous()  # [n_columns][n][2048]
    d_comm = block.comm[:n].contiguous()
    outs, plain = Outs(n), Outs(n, (False, False, True, True))
    torch.cuda.synchronize()
    assert ctx.recover_data_columns_checked_device(n, SETS[name], d_in.data_ptr(), d_comm.data_ptr(), **outs.ptrs()) == [0] * n
    outs.expect(block, range(n))
    assert ctx.recover_data_columns_device(n, SETS[name], d_in.data_ptr(), plain.cells.ptr, plain.proofs.ptr) == [0] * n
    torch.cuda.synchronize()
    assert torch.equal(outs.cells.body(), plain.cells.body()) and torch.equal(outs.proofs.body(), plain.proofs.body())


def test_byte_arrays_at_odd_addresses(ctx, block):
    """the device form's byte arrays may start at any byte address: commitments in and out, and the blobs, one byte off"""
    import torch
    n, idx = 3, SETS["random-64"]
    d_in = block.cells[:n].permute(1, 0, 2)[torch.tensor(idx, device="cuda")].contiguous()
    shifted = torch.zeros(n * PROOF + 1, dtype=torch.uint8, device="cuda")
    shifted[1:] = block.comm[:n].reshape(-1)
    out_comm, out_blobs = Guarded(n * PROOF + 1), Guarded(n * BLOB + 1)
    torch.cuda.synchronize()
    st = ctx.recover_data_columns_checked_device(n, idx, d_in.data_ptr(), shifted.data_ptr() + 1, d_out_blobs=out_blobs.ptr + 1,
                                                 d_out_commitments=out_comm.ptr + 1)
    torch.cuda.synchronize()
    assert st == [0] * n and out_comm.intact() and out_blobs.intact()
    assert torch.equal(out_comm.body()[1:].view(n, PROOF), block.comm[:n]) and torch.equal(out_blobs.body()[1:].view(n, BLOB), block.d_blobs[:n])
    assert int(out_comm.body()[0]) == 0x5A and int(out_blobs.body()[0]) == 0x5A


# ---- the gap the feature closes ----------------------------------------------------------------------------------------------------
def _both_forms(ctx, idx, given, comm, n, d_commitments=None):
    """-> (host form's result, device form's status, the device outputs)"""
    import torch
    host = ctx.recover_data_columns_checked(idx, given, comm, prefill=PRE)
    d_in = _device_input(given)
    d_comm = _device_bytes(comm) if comm is not None else None
    outs = Outs(n)
    torch.cuda.synchronize()
    st = ctx.recover_data_columns_checked_device(n, idx, d_in.data_ptr(), d_comm.data_ptr() if comm is not None else 0, **outs.ptrs())
    torch.cuda.synchronize()
    assert outs.intact()
    return host, st, outs


def test_sixty_four_columns_with_a_foreign_cell(ctx, block):
    """the reason for the call: exactly 64 columns decode to SOME polynomial whatever they hold"""
    n, idx = 3, SETS["random-64"]
    comm, cells, _ = _host_columns(block, n)
    foreign = _host_columns(block, 9)[1]
    given = [list(col) for col in B.cut_columns(cells, idx)]
    given[30][2] = foreign[idx[30]][8]  # blob 8's cell of that column in blob 2's place
    assert given[30][2] != cells[idx[30]][2]
    assert ctx.recover_data_columns(idx, given)[0] == [0, 0, 0]  # the unchecked call cannot tell
    host, st, outs = _both_forms(ctx, idx, given, comm, n)
    assert host[0] == st == [0, 0, 6]
    _expect_host(block, n, host[1:], skip={2})  # blobs 0 and 1 exact, blob 2's slots as they were
    outs.expect(block, range(n), skip={2})
    # without commitments nothing is compared: status 6 cannot occur
    assert ctx.recover_data_columns_checked(idx, given, None, want_blobs=False, want_cells=False, want_proofs=False)[0] == [0, 0, 0]


def test_wrong_commitments_on_right_cells(ctx, block):
    n, idx = 5, SETS["even"]
    comm, cells, _ = _host_columns(block, n)
    given = B.cut_columns(cells, idx)

    def statuses(c):
        host, st, outs = _both_forms(ctx, idx, given, c, n)
        assert host[0] == st
        bad = {i for i, s in enumerate(st) if s}
        _expect_host(block, n, host[1:], skip=bad)
        outs.expect(block, range(n), skip=bad)
        return st

    flipped = list(comm)
    flipped[3] = comm[3][:20] + bytes([comm[3][20] ^ 0x10]) + comm[3][21:]
    assert statuses(flipped) == [0, 0, 0, 6, 0]
    swapped = [comm[0], comm[2], comm[1], comm[3], comm[4]]
    assert statuses(swapped) == [0, 6, 6, 0, 0]
    malformed = [bytes([comm[0][0] & 0x7F]) + comm[0][1:]] + comm[1:]  # the compression flag cleared: never decoded, never equal
    assert statuses(malformed) == [6, 0, 0, 0, 0]
    assert statuses([comm[0], IDENTITY] + comm[2:]) == [0, 6, 0, 0, 0]  # the identity for a non-zero blob


def test_the_identity_matches_the_zero_blob_only(ctx, block):
    n, idx = 6, SETS["64-127"]
    comm, cells, _ = _host_columns(block, n)
    st = ctx.recover_data_columns_checked(idx, B.cut_columns(cells, idx), [IDENTITY] * n, want_blobs=False, want_commitments=False,
                                          want_cells=False, want_proofs=False)[0]
    assert st == [0 if i == ZERO_BLOB else 6 for i in range(n)]


# ---- order of checks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("right_commitment", [True, False])
def test_status_4_comes_before_6(ctx, block, right_commitment):
    n, idx = 3, SETS["65"]
    comm, cells, _ = _host_columns(block, n)
    foreign = _host_columns(block, 9)[1]
    given = [list(col) for col in B.cut_columns(cells, idx)]
    given[30][2] = foreign[idx[30]][8]  # 65 cells that lie on no polynomial of degree below 4096
    c = comm if right_commitment else comm[:2] + [comm[0]]
    host, st, outs = _both_forms(ctx, idx, given, c, n)
    assert host[0] == st == [0, 0, 4] == ctx.recover_data_columns(idx, given)[0]
    _expect_host(block, n, host[1:], skip={2})
    outs.expect(block, range(n), skip={2})


@pytest.mark.parametrize("right_commitment", [True, False])
def test_status_1_comes_before_6(ctx, block, right_commitment):
    n, idx = 3, SETS["random-64"]
    comm, cells, _ = _host_columns(block, n)
    given = [list(col) for col in B.cut_columns(cells, idx)]
    given[17][1] = given[17][1][:32 * 5] + NOT_CANONICAL + given[17][1][32 * 6:]
    c = comm if right_commitment else [comm[0], comm[2], comm[2]]
    host, st, outs = _both_forms(ctx, idx, given, c, n)
    assert host[0] == st == [0, 1, 0] == ctx.recover_data_columns(idx, given)[0]
    _expect_host(block, n, host[1:], skip={1})
    outs.expect(block, range(n), skip={1})


@pytest.mark.parametrize("idx", [list(range(63)), [1, 0] + list(range(2, 64)), list(range(63)) + [128]], ids=["63-columns", "descending", "index-128"])
def test_a_bad_index_list_marks_every_blob_3_and_writes_nothing(ctx, block, idx):
    import torch
    n = 3
    comm, cells, _ = _host_columns(block, n)
    given = [cells[c % CELLS] for c in idx]
    st, *got = ctx.recover_data_columns_checked(idx, given, comm, prefill=PRE)
    assert st == [3] * n
    _expect_host(block, n, got, skip={0, 1, 2})
    d_in = _device_input(given)
    host_comm = np.frombuffer(b"".join(comm), dtype=np.uint8).copy()  # HOST memory where device memory belongs: never resolved, never read
    outs = Outs(n)
    assert ctx.recover_data_columns_checked_device(n, idx, d_in.data_ptr(), host_comm.ctypes.data, **outs.ptrs()) == [3] * n
    torch.cuda.synchronize()
    assert outs.intact() and outs.untouched()


# ---- sub-batches, device lists, NULL outputs ---------------------------------------------------------------------------------------
def test_sub_batches_read_their_own_commitments(ctx64, block):
    import torch
    n, idx, bad = 70, SETS["random-64"], 66
    comm, cells, _ = _host_columns(block, n)
    wrong = list(comm)
    wrong[bad] = comm[0]
    want = [0] * 66 + [6] + [0] * 3
    d_in = block.cells[:n].permute(1, 0, 2)[torch.tensor(idx, device="cuda")].contiguous()
    d_comm = _device_bytes(wrong)
    outs = Outs(n)
    torch.cuda.synchronize()
    assert ctx64.recover_data_columns_checked_device(n, idx, d_in.data_ptr(), d_comm.data_ptr(), **outs.ptrs()) == want
    outs.expect(block, range(n), skip={bad})
    st, *got = ctx64.recover_data_columns_checked(idx, B.cut_columns(cells, idx), wrong, want_cells=False, want_proofs=False, prefill=PRE)
    assert st == want
    _expect_host(block, n, got, skip={bad}, want=(True, True, False, False))


def test_device_list_slices_by_blob(ctx, block):
    n, idx = 5, SETS["even"]
    comm, cells, _ = _host_columns(block, n)
    wrong = list(comm)
    wrong[3] = comm[4]  # in the second slice (blobs 2..4)
    two = _ctx(devices=[0, 0])
    try:
        st, *got = two.recover_data_columns_checked(idx, B.cut_columns(cells, idx), wrong, prefill=PRE)
        assert st == [0, 0, 0, 6, 0]
        _expect_host(block, n, got, skip={3})
    finally:
        two.close()


WANTS = [(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True), (False, False, True, True)]


@pytest.mark.parametrize("want", WANTS, ids=["blobs", "commitments", "cells", "proofs", "cells+proofs"])
def test_null_outputs_are_not_computed(ctx, block, want):
    import torch
    n, idx = 3, SETS["random-64"]
    comm, cells, _ = _host_columns(block, n)
    st, *got = ctx.recover_data_columns_checked(idx, B.cut_columns(cells, idx), comm, want_blobs=want[0], want_commitments=want[1],
                                                want_cells=want[2], want_proofs=want[3])
    assert st == [0] * n
    _expect_host(block, n, got, want=want)
    d_in = block.cells[:n].permute(1, 0, 2)[torch.tensor(idx, device="cuda")].contiguous()
    d_comm = block.comm[:n].contiguous()
    outs = Outs(n, want)
    torch.cuda.synchronize()
    assert ctx.recover_data_columns_checked_device(n, idx, d_in.data_ptr(), d_comm.data_ptr(), **outs.ptrs()) == [0] * n
    outs.expect(block, range(n))


def test_a_pure_check_runs_no_cell_kernel_and_no_fk20_stage(ctx, block):
    import torch
    n, idx = 9, SETS["random-64"]
    d_in = block.cells[:n].permute(1, 0, 2)[torch.tensor(idx, device="cuda")].contiguous()
    d_comm = block.comm[:n].contiguous()
    proofs, ref_proofs = Guarded(CELLS * n * PROOF), Guarded(CELLS * n * PROOF)
    torch.cuda.synchronize()
    launches = lambda t, stage: t[stage][1]  # noqa: E731
    ctx.set_profiling(1)
    try:
        ctx.get_stage_times()
        assert ctx.recover_data_columns_checked_device(n, idx, d_in.data_ptr(), d_comm.data_ptr()) == [0] * n
        pure = ctx.get_stage_times()
        assert ctx.recover_data_columns_checked_device(n, idx, d_in.data_ptr(), d_comm.data_ptr(), d_out_proofs=proofs.ptr) == [0] * n
        checked = ctx.get_stage_times()
        assert ctx.recover_data_columns_device(n, idx, d_in.data_ptr(), 0, ref_proofs.ptr) == [0] * n
        plain = ctx.get_stage_times()
    finally:
        ctx.set_profiling(0)
    assert launches(pure, "fk20_scalars") == 0 and launches(pure, "g1_linmap") == 0 and launches(pure, "coeffs_to_cells") == 0
    assert launches(pure, "compress") == 1
    assert launches(checked, "compress") == launches(plain, "compress") + 1  # the commitment's
    assert proofs.intact() and torch.equal(proofs.body(), ref_proofs.body())


# ---- streams and pointers ------------------------------------------------------------------------------------------------------------
def test_inputs_written_on_the_callers_stream(ctx, block):
    """d_cells and d_commitments filled by non-blocking copies from pinned memory on the caller's stream, the call on that stream with
    no synchronisation in between"""
    import torch
    n, idx = 7, SETS["random-64"]
    picks = list(range(20, 20 + n))
    comm, cells, _ = _host_columns(block, 27)
    given = [[cells[c][i] for i in picks] for c in idx]
    pin_cells = torch.from_numpy(np.frombuffer(B.flat(given), dtype=np.uint8).copy()).pin_memory()
    wrong = [comm[i] for i in picks]
    wrong[4] = comm[0]
    pin_comm = torch.from_numpy(np.frombuffer(b"".join(wrong), dtype=np.uint8).copy()).pin_memory()
    outs = Outs(n)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_cells = torch.empty(len(idx) * n * CELL, dtype=torch.uint8, device="cuda")
        d_comm = torch.empty(n * PROOF, dtype=torch.uint8, device="cuda")
        d_cells.copy_(pin_cells, non_blocking=True)
        d_comm.copy_(pin_comm, non_blocking=True)
    st = ctx.recover_data_columns_checked_device(n, idx, d_cells.data_ptr(), d_comm.data_ptr(), stream=s.cuda_stream, **outs.ptrs())
    assert st == [0, 0, 0, 0, 6, 0, 0]
    s.synchronize()
    outs.expect(block, picks, skip={4})


@pytest.mark.parametrize("which", ["d_commitments", "d_out_blobs", "d_out_commitments"])
def test_a_host_pointer_is_refused(ctx, block, which):
    import torch
    n, idx = 3, SETS["even"]
    d_in = block.cells[:n].permute(1, 0, 2)[torch.tensor(idx, device="cuda")].contiguous()
    d_comm = block.comm[:n].contiguous()
    outs = Outs(n)
    host = np.zeros(n * BLOB, dtype=np.uint8)
    args = dict(d_commitments=d_comm.data_ptr(), **outs.ptrs())
    args[which] = host.ctypes.data
    torch.cuda.synchronize()
    with pytest.raises(kzg.KzgError, match="InvalidInput"):
        ctx.recover_data_columns_checked_device(n, idx, d_in.data_ptr(), **args)
    torch.cuda.synchronize()
    assert outs.intact() and outs.untouched() and not host.any()


# ---- with the proposer's call ------------------------------------------------------------------------------------------------------
def test_round_trip_compute_then_checked_recovery(ctx, block):
    import torch
    n = 5
    comm, cells, proofs = Guarded(n * PROOF), Guarded(CELLS * n * CELL), Guarded(CELLS * n * PROOF)
    assert ctx.compute_data_columns_device(n, block.d_blobs.data_ptr(), comm.ptr, cells.ptr, proofs.ptr) == [0] * n
    torch.cuda.synchronize()
    held = sorted(random.Random("recover-checked:round-trip").sample(range(CELLS), 64))
    d_in = cells.body().view(CELLS, n, CELL)[torch.tensor(held, device="cuda")].contiguous()
    outs = Outs(n)
    torch.cuda.synchronize()
    assert ctx.recover_data_columns_checked_device(n, held, d_in.data_ptr(), comm.ptr, **outs.ptrs()) == [0] * n
    torch.cuda.synchronize()
    assert outs.intact()
    assert torch.equal(outs.cells.body(), cells.body()) and torch.equal(outs.proofs.body(), proofs.body())
    assert torch.equal(outs.comm.body(), comm.body()) and torch.equal(outs.blobs.body().view(n, BLOB), block.d_blobs[:n])
