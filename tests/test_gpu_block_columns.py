"""A block's data columns computed and recovered in column layout: eth_kzg_amd_compute_data_columns / _recover_data_columns, host and
device forms, against the blob-major calls of the same library transposed by tests/block_columns.py -- and, for the first three blobs,
against the CPU oracle directly, so that the library is not only compared with itself.

The contract is byte equality with calls that exist (c_eth_kzg.h), so every check is `==` on bytes; there are no tolerances.  The block
is 130 seeded blobs (synth.seeded_blob): its blob-major commitments, cells and proofs are computed ONCE on the GPU by
blob_to_kzg_commitment_device / compute_cells_and_kzg_proofs_device, kept there, and never changed; the tests take the first n.  The
shapes are the smallest at which each path can go wrong: 1 and 2 blobs the circulant form (four and two MSM segments), 3 the flat MSM, 9
and 17 two lanes per window with four and two lanes per blob in the linear map, 33 and 64 a full compress wave, 65 a second lane group
with one live lane; 70 and 130 under ETH_KZG_AMD_DEVICE_BATCH_MAX=64 give sub-batches 64 + 6 and 64 + 64 + 2 (b0 != 0, n_total != nb);
1990 blobs pad to a stride of 2048, the smallest at which the compress launcher takes four positions per thread, with 6 live lanes in
the last wave.  Device outputs lie between 4096 guard bytes of 0xA5 on either side."""
import ctypes as C
import importlib
import os
import random
import threading

import numpy as np
import pytest

import block_columns as B
import synth

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu

N_BLOCK, GUARD = 130, 4096
BLOB, CELL, PROOF, CELLS = 131072, 2048, 48, 128
NOT_CANONICAL = b"\xff" * 32  # >= r
COMPUTE_SIZES = [1, 2, 3, 9, 17, 33, 64, 65]


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


class Block:
    """the block in blob-major layout: host blobs, and the device tensors blobs [n][131072], comm [n][48], cells [n][128][2048], proofs [n][128][48]"""


@pytest.fixture(scope="module")
def block(ctx):
    import torch
    blk = Block()
    blk.blobs = [synth.seeded_blob(9100 + i) for i in range(N_BLOCK)]
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
    """(commitments[i], cells[c][i], proofs[c][i]) of the first n blobs as byte strings: the reference, transposed by the helper"""
    if n not in block._host:
        comm = block.comm[:n].cpu().numpy().tobytes()
        cells = B.unflat(block.cells[:n].cpu().numpy().tobytes(), n, CELLS, CELL)
        proofs = B.unflat(block.proofs[:n].cpu().numpy().tobytes(), n, CELLS, PROOF)
        block._host[n] = ([comm[PROOF * i:PROOF * i + PROOF] for i in range(n)], B.to_columns(cells), B.to_columns(proofs))
    return block._host[n]


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


def _outputs(n):
    return Guarded(n * PROOF), Guarded(CELLS * n * CELL), Guarded(CELLS * n * PROOF)


def _expect_block(block, n, comm, cells, proofs, blobs=None):
    """the three device outputs of a column call on the first n blobs (or on `blobs`, indices into the block) against the reference, permuted on the GPU"""
    import torch
    torch.cuda.synchronize()
    pick = slice(0, n) if blobs is None else torch.tensor(blobs, device="cuda")
    for g, ref, width in ((comm, None, PROOF), (cells, block.cells, CELL), (proofs, block.proofs, PROOF)):
        if g is None:
            continue
        assert g.intact()
        if ref is None:
            assert torch.equal(g.body().view(n, PROOF), block.comm[pick])
        else:
            assert torch.equal(g.body().view(CELLS, n, width), ref[pick].permute(1, 0, 2))


# ---- compute -------------------------------------------------------------------------------------------------------------------
def test_the_reference_block_equals_the_oracle_on_its_first_blobs(ctx, block):
    """n_blobs <= 3 also from the oracle directly: the blob-major reference every other test permutes, and the column call itself"""
    from oracle_lib import Oracle
    oracle = Oracle(use_precomp=True, threads=min(8, os.cpu_count() or 1))
    try:
        comm, cells, proofs = _host_columns(block, 3)
        st, got_comm, got_cells, got_proofs = ctx.compute_data_columns(block.blobs[:3])
        assert st == [0, 0, 0]
        for i in range(3):
            oc, op = oracle.compute_cells_and_kzg_proofs(block.blobs[i])
            assert [cells[c][i] for c in range(CELLS)] == oc and [proofs[c][i] for c in range(CELLS)] == op
            assert [got_cells[c][i] for c in range(CELLS)] == oc and [got_proofs[c][i] for c in range(CELLS)] == op
            assert comm[i] == got_comm[i] == oracle.blob_to_kzg_commitment(block.blobs[i])
    finally:
        oracle.close()


@pytest.mark.parametrize("n", COMPUTE_SIZES)
def test_compute_device_form(ctx, block, n):
    comm, cells, proofs = _outputs(n)
    st = ctx.compute_data_columns_device(n, block.d_blobs.data_ptr(), comm.ptr, cells.ptr, proofs.ptr)
    assert st == [0] * n
    _expect_block(block, n, comm, cells, proofs)


@pytest.mark.parametrize("n", COMPUTE_SIZES)
def test_compute_host_form(ctx, block, n):
    st, comm, cells, proofs = ctx.compute_data_columns(block.blobs[:n])
    assert st == [0] * n
    assert (comm, cells, proofs) == _host_columns(block, n)


@pytest.fixture(scope="module")
def ctx64():
    c = _ctx(ETH_KZG_AMD_DEVICE_BATCH_MAX="64")
    yield c
    c.close()


@pytest.mark.parametrize("n", [70, 130])
def test_sub_batches_write_their_blobs_of_every_column(ctx64, block, n):
    comm, cells, proofs = _outputs(n)
    assert ctx64.compute_data_columns_device(n, block.d_blobs.data_ptr(), comm.ptr, cells.ptr, proofs.ptr) == [0] * n
    _expect_block(block, n, comm, cells, proofs)


def test_four_positions_per_thread_compress_at_1990_blobs(ctx, block):
    """compared on the GPU with compute_cells_and_kzg_proofs_device and blob_to_kzg_commitment_device, permuted; one call each.  The
    blobs: seeded blob k % 130 with its field elements rotated by k // 130 places -- canonical elements, 1990 different blobs"""
    import torch
    n = 1990
    d_blobs = torch.stack([torch.roll(block.d_blobs[k % N_BLOCK].view(4096, 32), k // N_BLOCK, 0).reshape(BLOB) for k in range(n)]).contiguous()
    ref_comm = torch.zeros(n, PROOF, dtype=torch.uint8, device="cuda")
    ref_cells = torch.zeros(n, CELLS, CELL, dtype=torch.uint8, device="cuda")
    ref_proofs = torch.zeros(n, CELLS, PROOF, dtype=torch.uint8, device="cuda")
    comm, cells, proofs = _outputs(n)
    torch.cuda.synchronize()
    assert ctx.compute_data_columns_device(n, d_blobs.data_ptr(), comm.ptr, cells.ptr, proofs.ptr) == [0] * n
    assert ctx.compute_cells_and_kzg_proofs_device(n, d_blobs.data_ptr(), ref_cells.data_ptr(), ref_proofs.data_ptr()) == [0] * n
    assert ctx.blob_to_kzg_commitment_device(n, d_blobs.data_ptr(), ref_comm.data_ptr()) == [0] * n
    torch.cuda.synchronize()
    assert comm.intact() and cells.intact() and proofs.intact()
    assert torch.equal(comm.body().view(n, PROOF), ref_comm)
    assert torch.equal(proofs.body().view(CELLS, n, PROOF), ref_proofs.permute(1, 0, 2))
    assert torch.equal(cells.body().view(CELLS, n, CELL), ref_cells.permute(1, 0, 2))
    assert len({bytes(r) for r in ref_comm.cpu().numpy()}) == n  # (the blobs really differ)


@pytest.mark.parametrize("bad", [0, 2, 4])
def test_a_refused_blob_costs_its_own_slots_only(ctx, block, bad):
    import torch
    n = 5
    blobs = list(block.blobs[:n])
    blobs[bad] = blobs[bad][:32 * 77] + NOT_CANONICAL + blobs[bad][32 * 78:]
    want_st = [1 if i == bad else 0 for i in range(n)]
    ref_comm, ref_cells, ref_proofs = _host_columns(block, n)
    # host form: the refused blob's pre-filled buffers are untouched, every other byte is exact
    st, comm, cells, proofs = ctx.compute_data_columns(blobs, prefill=0xC3)
    assert st == want_st
    for i in range(n):
        if i == bad:
            assert comm[i] == b"\xc3" * PROOF
            assert all(cells[c][i] == b"\xc3" * CELL and proofs[c][i] == b"\xc3" * PROOF for c in range(CELLS))
        else:
            assert comm[i] == ref_comm[i]
            assert all(cells[c][i] == ref_cells[c][i] and proofs[c][i] == ref_proofs[c][i] for c in range(CELLS))
    # device form: its slots are unspecified, the others exact, the guards whole
    d_blobs = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).cuda()
    g_comm, g_cells, g_proofs = _outputs(n)
    assert ctx.compute_data_columns_device(n, d_blobs.data_ptr(), g_comm.ptr, g_cells.ptr, g_proofs.ptr) == want_st
    torch.cuda.synchronize()
    assert g_comm.intact() and g_cells.intact() and g_proofs.intact()
    others = torch.tensor([i for i in range(n) if i != bad], device="cuda")
    assert torch.equal(g_comm.body().view(n, PROOF)[others], block.comm[others])
    assert torch.equal(g_cells.body().view(CELLS, n, CELL)[:, others], block.cells[others].permute(1, 0, 2))
    assert torch.equal(g_proofs.body().view(CELLS, n, PROOF)[:, others], block.proofs[others].permute(1, 0, 2))


@pytest.mark.parametrize("want", [(True, False, False), (False, True, False), (False, False, True), (False, True, True)],
                         ids=["commitments", "cells", "proofs", "cells+proofs"])
def test_null_outputs_are_not_computed(ctx, block, want):
    n = 3
    ref = _host_columns(block, n)
    st, *got = ctx.compute_data_columns(block.blobs[:n], want_commitments=want[0], want_cells=want[1], want_proofs=want[2])
    assert st == [0] * n
    assert got == [r if w else None for r, w in zip(ref, want)]
    outs = [g if w else None for g, w in zip(_outputs(n), want)]
    assert ctx.compute_data_columns_device(n, block.d_blobs.data_ptr(), *[g.ptr if g else 0 for g in outs]) == [0] * n
    _expect_block(block, n, *outs)


def _async_call(ctx, block, picks, stream):
    """blobs copied on the caller's stream from pinned memory, the call on that stream without a status array: nothing has synchronised"""
    import torch
    n = len(picks)
    pinned = torch.from_numpy(np.frombuffer(b"".join(block.blobs[i] for i in picks), dtype=np.uint8).copy()).pin_memory()
    outs = _outputs(n)
    with torch.cuda.stream(stream):
        d = torch.empty(n * BLOB, dtype=torch.uint8, device="cuda")
        d.copy_(pinned, non_blocking=True)
    assert ctx.compute_data_columns_device(n, d.data_ptr(), outs[0].ptr, outs[1].ptr, outs[2].ptr, want_status=False, stream=stream.cuda_stream) is None
    return outs, (pinned, d)


def test_asynchronous_use_on_caller_streams(ctx, block):
    import torch
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    picks = list(range(20, 29))
    outs, keep = _async_call(ctx, block, picks, s1)
    s1.synchronize()
    _expect_block(block, len(picks), *outs, blobs=picks)
    # two calls on two streams
    pa, pb = list(range(40, 45)), list(range(60, 77))
    outs_a, keep_a = _async_call(ctx, block, pa, s1)
    outs_b, keep_b = _async_call(ctx, block, pb, s2)
    s1.synchronize()
    s2.synchronize()
    _expect_block(block, len(pa), *outs_a, blobs=pa)
    _expect_block(block, len(pb), *outs_b, blobs=pb)


def test_one_decode_feeds_commitments_and_proofs(ctx, block):
    """the stage marks of one column call at 9 blobs against compute_cells_and_kzg_proofs_device's"""
    n = 9
    comm, cells, proofs = _outputs(n)
    ref_cells, ref_proofs = Guarded(n * CELLS * CELL), Guarded(n * CELLS * PROOF)
    ctx.set_profiling(1)
    try:
        ctx.get_stage_times()
        assert ctx.compute_data_columns_device(n, block.d_blobs.data_ptr(), comm.ptr, cells.ptr, proofs.ptr) == [0] * n
        col = ctx.get_stage_times()
        assert ctx.compute_cells_and_kzg_proofs_device(n, block.d_blobs.data_ptr(), ref_cells.ptr, ref_proofs.ptr) == [0] * n
        ref = ctx.get_stage_times()
    finally:
        ctx.set_profiling(0)
    launches = lambda t, stage: t[stage][1]  # noqa: E731
    assert launches(col, "blob_to_coeffs") == 1 and launches(ref, "blob_to_coeffs") == 1
    assert launches(col, "coeffs_to_cells") == launches(ref, "coeffs_to_cells") >= 1
    assert launches(col, "compress") == launches(ref, "compress") + 1  # the commitment's
    _expect_block(block, n, comm, cells, proofs)


# ---- recover -------------------------------------------------------------------------------------------------------------------
def _column_sets():
    rng = random.Random("block-columns:held")
    return {"even": list(range(0, 128, 2)), "0-63": list(range(64)), "64-127": list(range(64, 128)), "random-64": sorted(rng.sample(range(128), 64)),
            "65": sorted(rng.sample(range(128), 65)), "127": sorted(rng.sample(range(128), 127)), "all": list(range(128))}


SETS = _column_sets()
_batch_reference = {}


def _recovered_by_the_batch_call(ctx, block, n, name):
    """recover_cells_and_kzg_proofs_batch on the expanded input, transposed; once per case, shared by the two forms"""
    if (n, name) not in _batch_reference:
        _, cells, _ = _host_columns(block, n)
        st, rc, rp = ctx.recover_cells_and_kzg_proofs_batch(B.expand_recovery(SETS[name], B.cut_columns(cells, SETS[name])))
        _batch_reference[(n, name)] = (st, B.to_columns(rc), B.to_columns(rp))
    return _batch_reference[(n, name)]


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("n", [1, 3, 65])
def test_recover_host_form(ctx, block, n, name):
    _, cells, proofs = _host_columns(block, n)
    st, got_cells, got_proofs = ctx.recover_data_columns(SETS[name], B.cut_columns(cells, SETS[name]))
    assert st == [0] * n
    assert (st, got_cells, got_proofs) == _recovered_by_the_batch_call(ctx, block, n, name)
    assert (got_cells, got_proofs) == (cells, proofs)  # the block the columns were cut from


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("n", [1, 3, 65])
def test_recover_device_form(ctx, block, n, name):
    import torch
    held = torch.tensor(SETS[name], device="cuda")
    d_in = block.cells[:n].permute(1, 0, 2)[held].contiguous()  # [n_columns][n][2048]
    out_cells, out_proofs = Guarded(CELLS * n * CELL), Guarded(CELLS * n * PROOF)
    torch.cuda.synchronize()
    assert ctx.recover_data_columns_device(n, SETS[name], d_in.data_ptr(), out_cells.ptr, out_proofs.ptr) == [0] * n
    _expect_block(block, n, None, out_cells, out_proofs)
    st, ref_cells, ref_proofs = _recovered_by_the_batch_call(ctx, block, n, name)
    assert st == [0] * n
    assert out_cells.body().cpu().numpy().tobytes() == B.flat(ref_cells) and out_proofs.body().cpu().numpy().tobytes() == B.flat(ref_proofs)


BAD_LISTS = {"63-columns": list(range(63)), "129-entries": list(range(128)) + [128], "descending-pair": [1, 0] + list(range(2, 64)),
             "repeated-index": [0, 0] + list(range(1, 63)), "index-128": list(range(63)) + [128]}


@pytest.mark.parametrize("name", list(BAD_LISTS))
def test_a_bad_index_list_marks_every_blob_3_and_writes_nothing(ctx, block, name):
    import torch
    n, idx = 3, BAD_LISTS[name]
    assert B.index_list_status(idx) == 3
    _, cells, _ = _host_columns(block, n)
    given = [cells[c % CELLS] for c in idx]
    st, got_cells, got_proofs = ctx.recover_data_columns(idx, given, prefill=0xC3)
    assert st == [3] * n
    assert all(x == b"\xc3" * CELL for col in got_cells for x in col) and all(x == b"\xc3" * PROOF for col in got_proofs for x in col)
    d_in = torch.from_numpy(np.frombuffer(B.flat(given), dtype=np.uint8).copy()).cuda()
    out_cells, out_proofs = Guarded(CELLS * n * CELL), Guarded(CELLS * n * PROOF)
    assert ctx.recover_data_columns_device(n, idx, d_in.data_ptr(), out_cells.ptr, out_proofs.ptr) == [3] * n
    torch.cuda.synchronize()
    assert out_cells.intact() and out_proofs.intact()
    assert bool((out_cells.body() == 0x5A).all()) and bool((out_proofs.body() == 0x5A).all())


def _recover_both_forms(ctx, idx, given, n):
    """-> (host form's result, device form's status, cells [128][n][2048] and proofs [128][n][48] as device tensors)"""
    import torch
    host = ctx.recover_data_columns(idx, given, prefill=0xC3)
    d_in = torch.from_numpy(np.frombuffer(B.flat(given), dtype=np.uint8).copy()).cuda()
    out_cells, out_proofs = Guarded(CELLS * n * CELL), Guarded(CELLS * n * PROOF)
    st = ctx.recover_data_columns_device(n, idx, d_in.data_ptr(), out_cells.ptr, out_proofs.ptr)
    torch.cuda.synchronize()
    assert out_cells.intact() and out_proofs.intact()
    return host, st, out_cells.body().view(CELLS, n, CELL), out_proofs.body().view(CELLS, n, PROOF)


def _others_exact(block, n, bad, host, d_cells, d_proofs):
    import torch
    _, cells, proofs = _host_columns(block, n)
    _, got_cells, got_proofs = host
    for i in range(n):
        if i == bad:
            assert all(got_cells[c][i] == b"\xc3" * CELL and got_proofs[c][i] == b"\xc3" * PROOF for c in range(CELLS))
        else:
            assert all(got_cells[c][i] == cells[c][i] and got_proofs[c][i] == proofs[c][i] for c in range(CELLS))
    others = torch.tensor([i for i in range(n) if i != bad], device="cuda")
    assert torch.equal(d_cells[:, others], block.cells[others].permute(1, 0, 2))
    assert torch.equal(d_proofs[:, others], block.proofs[others].permute(1, 0, 2))


def test_a_non_canonical_element_costs_its_blob_only(ctx, block):
    n, idx = 3, SETS["random-64"]
    _, cells, _ = _host_columns(block, n)
    given = [list(col) for col in B.cut_columns(cells, idx)]
    given[17][1] = given[17][1][:32 * 5] + NOT_CANONICAL + given[17][1][32 * 6:]
    host, st, d_cells, d_proofs = _recover_both_forms(ctx, idx, given, n)
    assert host[0] == st == [0, 1, 0]
    assert st == ctx.recover_cells_and_kzg_proofs_batch(B.expand_recovery(idx, given))[0]
    _others_exact(block, n, 1, host, d_cells, d_proofs)


def test_a_foreign_cell_costs_its_blob_only(ctx, block):
    n, idx = 3, SETS["65"]
    _, cells, _ = _host_columns(block, n)
    foreign = _host_columns(block, 9)[1]
    given = [list(col) for col in B.cut_columns(cells, idx)]
    given[30][2] = foreign[idx[30]][8]  # blob 8's cell of that column: 65 cells that lie on no polynomial of degree < 4096
    host, st, d_cells, d_proofs = _recover_both_forms(ctx, idx, given, n)
    assert host[0] == st == [0, 0, 4]
    assert st == ctx.recover_cells_and_kzg_proofs_batch(B.expand_recovery(idx, given))[0]
    _others_exact(block, n, 2, host, d_cells, d_proofs)


# ---- the three column calls together ----------------------------------------------------------------------------------------------
def test_round_trip_compute_verify_recover(ctx, block):
    import torch
    n = 5
    comm, cells, proofs = _outputs(n)
    assert ctx.compute_data_columns_device(n, block.d_blobs.data_ptr(), comm.ptr, cells.ptr, proofs.ptr) == [0] * n
    torch.cuda.synchronize()
    every = list(range(CELLS))
    for leaf in (False, True):
        ver, st = ctx.verify_data_columns_device(n, comm.ptr, every, cells.ptr, proofs.ptr, leaf_transcript=leaf)
        assert ver == [True] * CELLS and st == [0] * CELLS
    held = sorted(random.Random("block-columns:round-trip").sample(range(CELLS), 64))
    d_in = cells.body().view(CELLS, n, CELL)[torch.tensor(held, device="cuda")].contiguous()
    out_cells, out_proofs = Guarded(CELLS * n * CELL), Guarded(CELLS * n * PROOF)
    assert ctx.recover_data_columns_device(n, held, d_in.data_ptr(), out_cells.ptr, out_proofs.ptr) == [0] * n
    torch.cuda.synchronize()
    assert out_cells.intact() and out_proofs.intact()
    assert torch.equal(out_cells.body(), cells.body()) and torch.equal(out_proofs.body(), proofs.body())
    # one byte of one proof: exactly that column fails
    column, blob = 77, 3
    out_proofs.body().view(CELLS, n, PROOF)[column, blob, 20] ^= 1
    torch.cuda.synchronize()
    ver, _ = ctx.verify_data_columns_device(n, comm.ptr, every, out_cells.ptr, out_proofs.ptr, leaf_transcript=True)
    assert ver == [c != column for c in range(CELLS)]


# ---- device list and threads --------------------------------------------------------------------------------------------------------
def test_device_list_slices_by_blob_and_device_forms_run_on_the_owner(ctx, block):
    import torch
    n = 5
    two = _ctx(devices=[0, 0])
    try:
        ref = _host_columns(block, n)
        st, *got = two.compute_data_columns(block.blobs[:n])  # slices of 2 and 3 blobs write into the shared column arrays
        assert st == [0] * n and tuple(got) == ref
        idx = SETS["even"]
        st, rc, rp = two.recover_data_columns(idx, B.cut_columns(ref[1], idx))
        assert st == [0] * n and (rc, rp) == (ref[1], ref[2])
        assert two.recover_data_columns(BAD_LISTS["descending-pair"], B.cut_columns(ref[1], BAD_LISTS["descending-pair"]))[0] == [3] * n
        comm, cells, proofs = _outputs(n)
        assert two.compute_data_columns_device(n, block.d_blobs.data_ptr(), comm.ptr, cells.ptr, proofs.ptr) == [0] * n
        _expect_block(block, n, comm, cells, proofs)
        d_in = block.cells[:n].permute(1, 0, 2)[torch.tensor(idx, device="cuda")].contiguous()
        out_cells, out_proofs = Guarded(CELLS * n * CELL), Guarded(CELLS * n * PROOF)
        torch.cuda.synchronize()
        assert two.recover_data_columns_device(n, idx, d_in.data_ptr(), out_cells.ptr, out_proofs.ptr) == [0] * n
        _expect_block(block, n, None, out_cells, out_proofs)
        host_cells = np.zeros(len(idx) * n * CELL, dtype=np.uint8)
        for c in (two, ctx):  # a host pointer where device memory is expected: refused, never dereferenced on the GPU
            with pytest.raises(kzg.KzgError, match="InvalidInput"):
                c.recover_data_columns_device(n, idx, host_cells.ctypes.data, out_cells.ptr, out_proofs.ptr)
            with pytest.raises(kzg.KzgError, match="InvalidInput"):
                c.compute_data_columns_device(n, host_cells.ctypes.data, comm.ptr, cells.ptr, proofs.ptr)
        torch.cuda.synchronize()
        assert out_cells.intact() and out_proofs.intact()
    finally:
        two.close()


def test_four_threads_on_one_context(ctx, block):
    results, errors = {}, []

    def work(t):
        try:
            results[t] = ctx.compute_data_columns(block.blobs[10 * t:10 * t + 3])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors
    comm, cells, proofs = _host_columns(block, 33)
    for t in range(4):
        st, got_comm, got_cells, got_proofs = results[t]
        picks = range(10 * t, 10 * t + 3)
        assert st == [0, 0, 0] and got_comm == [comm[i] for i in picks]
        assert got_cells == [[cells[c][i] for i in picks] for c in range(CELLS)]
        assert got_proofs == [[proofs[c][i] for i in picks] for c in range(CELLS)]
