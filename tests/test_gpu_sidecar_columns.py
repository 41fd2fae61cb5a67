"""eth_kzg_amd_blobs_to_data_columns / _device: a block's data columns from blobs whose 128 cell proofs the caller holds, and
k_blob_to_columns, the kernel behind the call without its flag.

Expected values come from the reference vectors, from the CPU oracle and from the calls that exist without this one --
compute_data_columns, compute_cells_and_kzg_proofs_batch, verify_blob_cell_proofs_many -- never from the new call; the expected matrices
are plain transpositions (tests/sidecar_columns.py).  Outputs lie over a guard pattern: what a call must not write shows.  The context
is test_gpu_blob_cells.py's (two host threads: passes of up to four items take the short-chain form, larger ones fold).  Host and
device form unless said otherwise.

1. The kernel alone through its hook, byte for byte against the oracle's compute_cells transposed: n = 1, n = 3, n = 3 as blobs 2..4 of
   5, a refused blob at position 1 of 3; the host form's launch (rows 0..63 not written).
2. flags = 0: 1, 3 and 5 blobs against compute_data_columns (and the oracle up to 3); random bytes as proofs; a refused blob in the
   middle; each output NULL in turn.
3. The reference vectors of compute_cells_and_kzg_proofs as the items of one flagged call.
4. The flag: verdicts and statuses item by item equal verify_blob_cell_proofs_many; 7 items (folded, searched) and 2 (short chain);
   outputs exactly for the items that pass.
5. Cuts: 200 items over 4 blobs, wrong proofs at 0, 199 and either side of the first cut.
6. Device form: odd byte offsets, a host pointer among the device pointers, inputs written on the caller's stream, the asynchronous return.
7. A device list 0,0."""
import importlib

import numpy as np
import pytest

import blob_cells as BC
import sidecar_columns as SC
import synth
import test_gpu_blob_cells as TB
import test_gpu_many_leaf as TL
import vectors
from verify_transcript import MANY_HOST_THREADS, off_subgroup_point

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu
R, INF, N = BC.R, BC.INF, BC.N_CELLS
G = SC.GUARD
_cache = {}  # material and expected values: computed once, shared by the tests, never changed


@pytest.fixture(scope="module")
def ctx():
    c = TL._ctx(ETH_KZG_AMD_HOST_THREADS=str(MANY_HOST_THREADS))
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool(ctx):
    """five distinct valid items (blob, commitment, 128 proofs) and the cells of every blob used, from the library's prover"""
    if "pool" not in _cache:
        blobs = [synth.seeded_blob(860 + b) for b in range(5)]
        st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(blobs)
        assert st == [0] * 5
        items = [(blobs[b], ctx.blob_to_kzg_commitment(blobs[b]), list(proofs[b])) for b in range(5)]
        cells_of = {blobs[b]: list(cells[b]) for b in range(5)}
        cells_of[bytes(BC.BLOB_BYTES)] = [bytes(BC.CELL_BYTES)] * N
        _cache["pool"] = (items, cells_of)
    return _cache["pool"]


def run(ctx, items, where, verify, want_cells=True, want_proofs=True, shift=0):
    """-> (verified, status, cells[c][i], proofs[c][i]) over the guard pattern"""
    if where == "host":
        return ctx.blobs_to_data_columns(items, verify=verify, want_cells=want_cells, want_proofs=want_proofs, prefill=G)
    d = SC.DeviceCall(items, shift=shift, want_cells=want_cells, want_proofs=want_proofs)
    ver, st = d.call(ctx, verify=verify)
    return ver, st, d.cells(), d.proofs()


def check_outputs(where, got_cells, got_proofs, items, cells_of, passed):
    """the slots of the items that passed hold their cells and their proofs; in the host form every other slot is on the guard pattern"""
    n = len(items)
    for c in range(N):
        for i in range(n):
            if passed[i]:
                assert got_cells is None or got_cells[c][i] == cells_of[items[i][0]][c], ("cell", where, c, i)
                assert got_proofs is None or got_proofs[c][i] == items[i][2][c], ("proof", where, c, i)
            elif where == "host":
                assert got_cells is None or got_cells[c][i] == SC.guard(SC.CELL_BYTES), ("cell written", c, i)
                assert got_proofs is None or got_proofs[c][i] == SC.guard(SC.PROOF_BYTES), ("proof written", c, i)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------
def _oracle_cells(oracle, blob):
    key = ("oracle", blob)
    if key not in _cache:
        _cache[key] = list(oracle.compute_cells(blob))
        assert _cache[key][:N // 2] == BC.blob_cells(blob)
    return _cache[key]


def _kernel_blobs():
    a, b = synth.seeded_blob(871), synth.seeded_blob(872)
    return [a, b, (R - 1).to_bytes(32, "big") * 4096, bytes(BC.BLOB_BYTES), BC.monomial_blob(4095)], [BC.with_element(a, 1024, R), BC.with_element(b, 4095, (1 << 256) - 1)]


@pytest.mark.parametrize("shape", ["n1", "n3", "n3-of-5-at-2", "refused-at-1-of-3", "host-form-launch"])
def test_the_kernel_alone_against_the_oracle(ctx, oracle, shape):
    good, bad = _kernel_blobs()
    if shape == "n1":
        launches = [([g], 1, 0, True) for g in good] + [([x], 1, 0, True) for x in bad]
    elif shape == "n3":
        launches = [(good[:3], 3, 0, True), (good[2:5], 3, 0, True)]
    elif shape == "n3-of-5-at-2":
        launches = [(good[1:4], 5, 2, True)]
    elif shape == "refused-at-1-of-3":
        launches = [([good[0], bad[0], good[1]], 3, 0, True), ([good[4], bad[1], good[3]], 5, 1, True)]
    else:
        launches = [([good[0], bad[0], good[1]], 4, 1, False)]
    for blobs, n_total, b0, blob_half in launches:
        matrix, flags = ctx.test_blob_to_columns(blobs, n_total=n_total, b0=b0, blob_half=blob_half, guard=G)
        assert flags == [1 if BC.blob_is_bad(x) else 0 for x in blobs], shape
        want = [[SC.guard(SC.CELL_BYTES)] * n_total for _ in range(N)]
        for i, blob in enumerate(blobs):
            if not BC.blob_is_bad(blob):
                cells = _oracle_cells(oracle, blob)
                for c in range(0 if blob_half else N // 2, N):
                    want[c][b0 + i] = cells[c]
        wrong = [(c, j) for c in range(N) for j in range(n_total) if matrix[c][j] != want[c][j]]
        assert not wrong, (shape, n_total, b0, wrong[:8])


def test_the_hook_refuses_a_launch_outside_its_matrix():
    lib = kzg.load_library()
    one = (np.zeros(1, dtype=np.uint64)).ctypes.data
    assert lib.eth_kzg_amd_test_blob_to_columns(None, 1, None, 1, 0, 1, None, None) == 3
    for n, n_total, b0 in ((3, 5, 3), (1, 1, 1), (2, 1, 0), (0, 1, 0), (1025, 2048, 0), (1, 4097, 0), (1, 5, (1 << 64) - 1)):
        assert lib.eth_kzg_amd_test_blob_to_columns(None, n, one, n_total, b0, 1, one, one) == 3, (n, n_total, b0)


# ---- 2. flags = 0 -----------------------------------------------------------------------------------------------------------------------------
def _random_proofs(seed):
    rng = np.random.default_rng(seed)
    return [rng.bytes(48) for _ in range(N)]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_without_the_flag_cells_are_compute_data_columns_and_proofs_are_copied(ctx, oracle, pool, where, n):
    good, cells_of = pool
    items = [(good[i][0], None, _random_proofs(40 + i)) for i in range(n)]  # never decoded: garbage is copied as garbage
    key = ("columns", n)
    if key not in _cache:
        st, _, cells, _ = ctx.compute_data_columns([it[0] for it in items], want_commitments=False, want_proofs=False)
        assert st == [0] * n
        _cache[key] = cells
    ver, st, cells, proofs = run(ctx, items, where, verify=False)
    assert ver is None and st == [0] * n
    assert cells == _cache[key]
    if n <= 3:
        assert cells == SC.transposed([_oracle_cells(oracle, it[0]) for it in items])
    assert proofs == SC.transposed([it[2] for it in items])


@pytest.mark.parametrize("where", ["host", "device"])
def test_without_the_flag_a_refused_blob_in_the_middle_and_each_output_null(ctx, pool, where):
    good, cells_of = pool
    bad_blob = BC.with_element(good[1][0], 2049, R)
    items = [(good[0][0], None, good[0][2]), (bad_blob, None, _random_proofs(7)), (good[2][0], None, _random_proofs(8))]
    if "refused" not in _cache:
        _cache["refused"] = ctx.compute_data_columns([it[0] for it in items], want_commitments=False, want_proofs=False)[0]
    assert _cache["refused"] == [0, 1, 0]
    for want_cells, want_proofs in ((True, True), (False, True), (True, False)):
        ver, st, cells, proofs = run(ctx, items, where, verify=False, want_cells=want_cells, want_proofs=want_proofs)
        assert ver is None and st == _cache["refused"], (want_cells, want_proofs)
        assert (cells is None) == (not want_cells) and (proofs is None) == (not want_proofs)
        check_outputs(where, cells, proofs, items, cells_of, [True, False, True])


# ---- 3. the reference vectors -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_reference_vectors_in_one_flagged_call(ctx, where):
    items, want, cells_of = [], [], {}
    for name, case in sorted(vectors.load("compute_cells_and_kzg_proofs").items()):
        blob = case["input"]["blob"]
        if len(blob) != BC.BLOB_BYTES:
            assert case["output"] is None, name
            continue
        if case["output"] is None:  # a well-formed blob with an element >= r: refused, whatever the points are
            assert BC.blob_is_bad(blob), name
            items.append((blob, INF, [INF] * N))
            want.append((False, 1))
        else:
            key = ("commitment", blob)
            if key not in _cache:
                _cache[key] = ctx.blob_to_kzg_commitment(blob)
            items.append((blob, _cache[key], list(case["output"][1])))
            cells_of[blob] = list(case["output"][0])
            want.append((True, 0))
    assert (True, 0) in want and (False, 1) in want and len(items) >= 3
    ver, st, cells, proofs = run(ctx, items, where, verify=True)
    assert list(zip(ver, st)) == want
    check_outputs(where, cells, proofs, items, cells_of, ver)


# ---- 4. the flag: the verdicts of verify_blob_cell_proofs_many, outputs for the items that pass ------------------------------------------------
def _flagged_items(pool, n):
    good, _ = pool
    a, b = good[0], good[1]
    off = off_subgroup_point()
    bad_blob = BC.with_element(a[0], 2049, R)
    if n == 2:
        return [good[2], TB.with_proof(a, 0, b[2][0])]
    return [a,
            TB.with_proof(a, 0, b[2][0]),          # wrong proof at k = 0
            TB.with_proof(good[3], 127, b[2][127]),  # wrong proof at k = 127
            (a[0], off, a[2]),                     # commitment off the subgroup
            TB.with_proof(b, 3, off),              # a proof off the subgroup
            (bad_blob, off, a[2]),                 # a non-canonical blob together with a bad point: status 1 wins
            (bytes(BC.BLOB_BYTES), INF, [INF] * N)]  # the all-zero blob with 129 identities


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", [7, 2])
def test_the_flag_gives_the_verdicts_of_the_existing_call_and_writes_what_passes(ctx, pool, where, n):
    items = _flagged_items(pool, n)
    key = ("verdicts", n)
    if key not in _cache:
        _cache[key] = ctx.verify_blob_cell_proofs_many(items)
        assert _cache[key] == TB.DeviceItems(items).call(ctx)
    want_ver, want_st = _cache[key]
    assert (want_ver, want_st) == (([True, False, False, False, False, False, True], [0, 0, 0, 2, 2, 1, 0]) if n == 7 else ([True, False], [0, 0]))
    ver, st, cells, proofs = run(ctx, items, where, verify=True)
    assert (ver, st) == (want_ver, want_st)
    check_outputs(where, cells, proofs, items, pool[1], want_ver)
    for want_cells, want_proofs in ((False, True), (True, False), (False, False)):  # each output NULL: the other is still correct
        ver, st, cells, proofs = run(ctx, items, where, verify=True, want_cells=want_cells, want_proofs=want_proofs)
        assert (ver, st) == (want_ver, want_st)
        check_outputs(where, cells, proofs, items, pool[1], want_ver)


# ---- 5. cuts ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_200_items_over_four_blobs_and_the_first_cut(ctx, pool, where):
    good, cells_of = pool
    n, first_cut = 200, BC.parts(200)[1]
    assert BC.parts(n) == [0, 67, 134, 200]
    wrong = [0, first_cut - 1, first_cut, 199]
    items = [good[i % 4] for i in range(n)]  # the same four objects: the host form's blob pointers alias four buffers
    for i in wrong:
        items[i] = TB.wrong_of(good[:4], i % 4, k=(i * 37) % N)
    if "cuts" not in _cache:
        _cache["cuts"] = ctx.verify_blob_cell_proofs_many(items)
    want_ver, want_st = _cache["cuts"]
    assert want_st == [0] * n and [i for i in range(n) if not want_ver[i]] == wrong
    ver, st, cells, proofs = run(ctx, items, where, verify=True)
    assert (ver, st) == (want_ver, want_st)
    check_outputs(where, cells, proofs, items, cells_of, want_ver)


# ---- 6. device form details -------------------------------------------------------------------------------------------------------------------
def test_device_arrays_at_odd_offsets(ctx, pool):
    items = _flagged_items(pool, 7)
    want = _cache.get(("verdicts", 7)) or ctx.verify_blob_cell_proofs_many(items)
    d = SC.DeviceCall(items, shift=13)
    assert d.inputs[1] % 2 == 1 and d.inputs[2] % 2 == 1 and d.out[1][1] % 2 == 1 and d.inputs[0] % 4 == 0 and d.inputs[0] % 16 != 0
    assert d.out[0][1] % 4 == 0 and d.out[0][1] % 16 != 0
    assert d.call(ctx, verify=True) == want
    check_outputs("device", d.cells(), d.proofs(), items, pool[1], want[0])
    plain = [(it[0], None, it[2]) for it in items[:3]]
    d = SC.DeviceCall(plain, shift=13)
    assert d.call(ctx) == (None, [0, 0, 0])
    check_outputs("device", d.cells(), d.proofs(), plain, pool[1], [True] * 3)


def test_a_host_pointer_among_the_device_pointers_is_an_error(ctx, pool):
    items = [pool[0][0], pool[0][1]]
    d = SC.DeviceCall(items)
    host = np.zeros(N * 2 * SC.CELL_BYTES, dtype=np.uint8)
    ptrs = [d.inputs[0], d.inputs[1], d.inputs[2], d.out[0][1], d.out[1][1]]
    for verify, holes in ((True, (0, 1, 2, 3, 4)), (False, (0, 2, 3, 4))):  # (without the flag the commitments are not read: not resolved)
        for h in holes:
            p = list(ptrs)
            p[h] = host.ctypes.data
            with pytest.raises(kzg.KzgError, match="InvalidInput"):
                ctx.blobs_to_data_columns_device(2, *p, verify=verify)
    assert not host.any()


def test_inputs_written_on_the_callers_stream_and_the_asynchronous_return(ctx, pool):
    import torch
    good, cells_of = pool
    items = [good[0], TB.with_proof(good[1], 64, good[0][2][64]), good[2]]
    plain = [(it[0], None, it[2]) for it in items]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # something in front of the writes, so that they have not happened when the call is made
        a = torch.randn(4096, 4096, device="cuda")
        for _ in range(8):
            a = a @ a
            a = a / a.abs().max()
    d = SC.DeviceCall(items, stream=s)
    assert d.call(ctx, verify=True, stream=s.cuda_stream) == ([True, False, True], [0, 0, 0])
    check_outputs("device", d.cells(), d.proofs(), items, cells_of, [True, False, True])
    with torch.cuda.stream(s):
        for _ in range(8):
            a = a @ a
            a = a / a.abs().max()
    d2 = SC.DeviceCall(plain, stream=s)
    assert d2.call(ctx, want_status=False, stream=s.cuda_stream) == (None, None)  # returns without synchronising
    s.synchronize()
    check_outputs("device", d2.cells(), d2.proofs(), plain, cells_of, [True] * 3)
    d3 = SC.DeviceCall(plain, stream=s)
    assert d3.call(ctx, stream=s.cuda_stream) == (None, [0, 0, 0])  # with status: complete on return
    check_outputs("device", d3.cells(), d3.proofs(), plain, cells_of, [True] * 3)
    torch.cuda.synchronize()


# ---- 7. a device list ---------------------------------------------------------------------------------------------------------------------------
def test_device_list_0_0(ctx, pool):
    good, cells_of = pool
    items = [good[0], TB.wrong_of(good[:4], 1), (BC.with_element(good[2][0], 7, R), good[2][1], good[2][2]), good[3], (good[1][0], INF, good[1][2])]
    want = ([True, False, False, True, False], [0, 0, 1, 0, 0])
    assert ctx.verify_blob_cell_proofs_many(items) == want
    plain = [(it[0], None, it[2]) for it in items]
    c2 = TL._ctx(devices=[0, 0], ETH_KZG_AMD_HOST_THREADS=str(MANY_HOST_THREADS))
    try:
        for c in (c2, ctx):  # cut by blob over the list: the same bytes and verdicts as on one device
            ver, st, cells, proofs = run(c, items, "host", verify=True)
            assert (ver, st) == want
            check_outputs("host", cells, proofs, items, cells_of, want[0])
            ver, st, cells, proofs = run(c, plain, "host", verify=False)
            assert ver is None and st == [0, 0, 1, 0, 0]
            check_outputs("host", cells, proofs, plain, cells_of, [True, True, False, True, True])
        d = SC.DeviceCall(items)
        assert d.call(c2, verify=True) == want
        check_outputs("device", d.cells(), d.proofs(), items, cells_of, want[0])
    finally:
        c2.close()
