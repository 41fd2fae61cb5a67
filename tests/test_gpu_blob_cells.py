"""eth_kzg_amd_verify_blob_cell_proofs_many / _many_device: many blobs against their 128 cell proofs per call, a verdict and a status for
each; and k_blob_to_extension, the kernel that feeds the pass.

Expected values come from the vectors, from the CPU oracle, from eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex (leaf flag) on the
expanded input (tests/blob_cells.py: the call this one must agree with) and from the statement in hashlib (tests/many_leaf.py).  The
hook eth_kzg_amd_test_verify_blob_cell_proofs_sums runs the public call's launches with the tap of
eth_kzg_amd_test_verify_many_sums_device.  The context has two host threads (test_gpu_many_leaf.py's): passes of up to four items take
the short-chain form, larger ones fold.  Host and device form unless said otherwise.

1. The kernel alone, byte for byte against the oracle's compute_cells and ctx.compute_cells, n = 1 and n = 3; refused blobs.
2. The reference vectors of compute_cells_and_kzg_proofs as the items of one call.
3. Verdicts and the order of errors, item by item against _many_ex on the expanded input; n = 1.
4. The statement byte for byte: the tap against the tap of the expanded pass and against hashlib; 7 items (folded, searched), 2 (short chain).
5. Cuts: 200 items over 4 blobs (three parts), wrong proofs at 0, 199 and either side of the first cut.
6. Device form: odd byte offsets, a host pointer or a mix is an error, blobs written on the caller's stream are seen.
7. A device list 0,0.
8. Four threads next to compute_cells_and_kzg_proofs on one context: no big lock, same results."""
import ctypes as C
import importlib
import threading

import numpy as np
import pytest

import blob_cells as BC
import many_leaf as M
import oracle_lib
import synth
import test_gpu_many_leaf as TL
import vectors
from verify_transcript import MANY_HOST_THREADS, off_subgroup_point

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu
R, INF, N = BC.R, BC.INF, BC.N_CELLS
LEAF = TL.LEAF
_cache = {}  # material and expected values: computed once, shared by the tests, never changed


@pytest.fixture(scope="module")
def ctx():
    c = TL._ctx(ETH_KZG_AMD_HOST_THREADS=str(MANY_HOST_THREADS))
    yield c
    c.close()


class DeviceItems:
    """the three flat arrays of a list of items in device memory; commitments and proofs `shift` bytes into their allocations, the blobs
    at the next multiple of four"""

    def __init__(self, items, shift=0, stream=None):
        import torch
        cols = [b"".join(it[0] for it in items), b"".join(it[1] for it in items), b"".join(p for it in items for p in it[2])]
        self.n, self.keep, self.ptrs = len(items), [], []
        for k, col in enumerate(cols):
            off = ((shift + 3) // 4 * 4 + 4 if shift else 0) if k == 0 else shift  # (13 -> 20: a multiple of 4 and not of 16)
            a = torch.from_numpy(np.frombuffer(col or bytes(1), dtype=np.uint8).copy())
            if stream is None:
                d = torch.empty(off + len(a), dtype=torch.uint8, device="cuda")
                d[off:].copy_(a)
            else:  # written by a kernel queued on the caller's stream: the call must wait for it
                with torch.cuda.stream(stream):
                    staged = a.pin_memory().to("cuda", non_blocking=True)
                    d = torch.zeros(off + len(a), dtype=torch.uint8, device="cuda")
                    d[off:] = staged ^ 0  # an elementwise kernel, not a copy engine
                self.keep.append(staged)
            self.keep.append(d)
            self.ptrs.append(d.data_ptr() + off)
        if stream is None:
            torch.cuda.synchronize()

    def call(self, ctx, stream=None):
        return ctx.verify_blob_cell_proofs_many_device(self.n, *self.ptrs, stream=stream)


def run(ctx, items, where):
    if where == "host":
        return ctx.verify_blob_cell_proofs_many(items)
    return DeviceItems(items).call(ctx)


# ---- material ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(ctx):
    """four distinct valid items (blob, commitment, 128 proofs) and their cells, from the library's prover"""
    if "pool" not in _cache:
        blobs = [synth.seeded_blob(60 + b) for b in range(4)]
        st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(blobs)
        assert st == [0] * 4
        items = [(blobs[b], ctx.blob_to_kzg_commitment(blobs[b]), list(proofs[b])) for b in range(4)]
        _cache["pool"] = (items, {blobs[b]: list(cells[b]) for b in range(4)})
        _cache["pool"][1][bytes(BC.BLOB_BYTES)] = [bytes(BC.CELL_BYTES)] * N
    return _cache["pool"]


def with_proof(item, k, proof):
    return (item[0], item[1], item[2][:k] + [proof] + item[2][k + 1:])


def wrong_of(good, i, k=5):
    """item i with another blob's proof for cell k"""
    return with_proof(good[i], k, good[(i + 1) % len(good)][2][k])


def expect_expanded(ctx, items, cells_of):
    """(verified, status) item by item: _many_ex with the leaf flag on the expanded input; a refused blob has no cells and is status 1"""
    live = [i for i, it in enumerate(items) if not BC.blob_is_bad(it[0])]
    ver, st = ctx.verify_cell_kzg_proof_batch_many([BC.expand(items[i], cells_of[items[i][0]]) for i in live], leaf_transcript=True)
    out_v, out_s = [False] * len(items), [1] * len(items)
    for j, i in enumerate(live):
        out_v[i], out_s[i] = ver[j], st[j]
    return out_v, out_s


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------
def _kernel_blobs():
    good = {"seeded-a": synth.seeded_blob(71), "seeded-b": synth.seeded_blob(72), "zero": bytes(BC.BLOB_BYTES),
            "all-r-minus-1": (R - 1).to_bytes(32, "big") * 4096}
    for j in (0, 1, 63, 64, 4095):
        good["monomial-%d" % j] = BC.monomial_blob(j)
    bad = {}
    for at in (0, 1023, 1024, 4095):
        bad["r-at-%d" % at] = BC.with_element(good["seeded-a"], at, R)
        bad["max-at-%d" % at] = BC.with_element(good["seeded-b"], at, (1 << 256) - 1)
    return good, bad


def _expected_cells(ctx, oracle, name, blob, refused):
    if name not in _cache:
        if refused:
            with pytest.raises(kzg.KzgError):
                ctx.compute_cells(blob)
            _cache[name] = BC.blob_cells(blob) + [bytes(BC.CELL_BYTES)] * (N // 2)
        else:
            want = list(oracle.compute_cells(blob))
            assert list(ctx.compute_cells(blob)) == want and want[:N // 2] == BC.blob_cells(blob), name
            _cache[name] = want
    return _cache[name]


def test_the_kernel_alone_against_the_oracle(ctx, oracle):
    good, bad = _kernel_blobs()
    every = [(k, v, False) for k, v in good.items()] + [(k, v, True) for k, v in bad.items()]
    assert len(every) == 17
    groups = [[e] for e in every]  # n = 1
    mixed = every[:9:2] + every[9:] + every[1:9:2]  # n = 3: refused and accepted blobs in one launch
    groups += [mixed[i:i + 3] for i in range(0, len(mixed) - 2, 3)]
    assert any(len({r for _, _, r in g}) == 2 for g in groups)
    for g in groups:
        cells, flags = ctx.test_blob_extension([b for _, b, _ in g])
        assert flags == [1 if r else 0 for _, _, r in g], [k for k, _, _ in g]
        for (name, blob, refused), got in zip(g, cells):
            want = _expected_cells(ctx, oracle, name, blob, refused)
            wrong = [k for k in range(N) if got[k] != want[k]]
            assert not wrong, (name, len(g), wrong[:8])


# ---- 2. the reference vectors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_reference_vectors_in_one_call(ctx, where):
    items, want = [], []
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
            want.append((True, 0))
    assert (True, 0) in want and len(items) >= 3
    ver, st = run(ctx, items, where)
    assert list(zip(ver, st)) == want


# ---- 3. verdicts and the order of errors ------------------------------------------------------------------------------------------------------
def _shapes(pool):
    good, _ = pool
    a, b = good[0], good[1]
    off_curve = next(c for c in (bytes([0x80]) + x.to_bytes(47, "big") for x in range(1, 64)) if oracle_lib.g1_validate(c, False) != 0)
    off = off_subgroup_point()
    assert oracle_lib.g1_validate(off, False) == 0 and oracle_lib.g1_validate(off, True) != 0
    bad_blob = BC.with_element(a[0], 2049, R)
    swapped = a[2][:]
    swapped[17], swapped[90] = swapped[90], swapped[17]
    return {
        "valid": (a, 0, True),
        "wrong-proof-at-0": (with_proof(a, 0, b[2][0]), 0, False),
        "wrong-proof-at-63": (with_proof(a, 63, b[2][63]), 0, False),
        "wrong-proof-at-64": (with_proof(a, 64, b[2][64]), 0, False),
        "wrong-proof-at-127": (with_proof(a, 127, b[2][127]), 0, False),
        "two-proofs-swapped": ((a[0], a[1], swapped), 0, False),
        "another-blobs-commitment": ((a[0], b[1], a[2]), 0, False),
        "proof-off-the-curve": (with_proof(a, 100, off_curve), 2, False),
        "proof-off-the-subgroup": (with_proof(a, 3, off), 2, False),
        "commitment-off-the-subgroup": ((a[0], off, a[2]), 2, False),
        "blob-bad-everything-else-valid": ((bad_blob, a[1], a[2]), 1, False),
        "blob-bad-and-a-bad-point": ((bad_blob, off, with_proof(a, 64, off_curve)[2]), 1, False),
        "zero-blob-with-identities": ((bytes(BC.BLOB_BYTES), INF, [INF] * N), 0, True),
        "another-valid": (b, 0, True),
    }


@pytest.mark.parametrize("where", ["host", "device"])
def test_order_of_errors_item_by_item_against_the_expanded_call(ctx, pool, where):
    shapes = _shapes(pool)
    items = [s[0] for s in shapes.values()]
    assert [BC.item_status(it) for it in items] == [s[1] for s in shapes.values()]  # the statement's order is the issue's
    if "shapes" not in _cache:
        _cache["shapes"] = expect_expanded(ctx, items, pool[1])
    want = _cache["shapes"]
    assert want == ([s[2] for s in shapes.values()], [s[1] for s in shapes.values()])
    assert run(ctx, items, where) == want
    for i in (0, 2, 8, 10, 11, 12):  # and alone: the short-chain form
        assert run(ctx, [items[i]], where) == ([want[0][i]], [want[1][i]]), i
    assert ctx.verify_blob_cell_proofs_many([]) == ([], []) and ctx.verify_blob_cell_proofs_many_device(0, 0, 0, 0) == ([], [])


# ---- 4. the statement, byte for byte ---------------------------------------------------------------------------------------------------------
def sums(ctx, items, where, max_probes=256):
    """eth_kzg_amd_test_verify_blob_cell_proofs_sums -> (return code, what test_gpu_many_leaf.many_sums hands out)"""
    lib = kzg.load_library()
    n = len(items)
    ver, st, form = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int32 * 4)()
    sm, rho, fold = C.create_string_buffer(96 * n), (C.c_uint32 * (4 * n))(), C.create_string_buffer(96)
    pr, ps, npr = (C.c_int32 * (3 * max_probes))(), C.create_string_buffer(96 * max_probes), C.c_uint64(0)
    dig, leaves = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n * N)
    if where == "host":
        ba, ca, pa, keep = ctx._marshal_blob_cell_proofs(items)
        src = [a.ctypes.data_as(C.c_void_p) for a in (ba, ca, pa)]
    else:
        keep = DeviceItems(items)
        src = [C.c_void_p(p) for p in keep.ptrs]
    rc = lib.eth_kzg_amd_test_verify_blob_cell_proofs_sums(ctx.handle, n, 0 if where == "host" else 1, *src, ver, st, form, sm, rho, fold, pr, ps,
                                                           max_probes, C.byref(npr), dig, leaves)
    del keep
    out = TL.ManySums()
    out.verified, out.status = [bool(v) for v in ver], list(st)
    out.small, out.folded, out.searched, out.fold_verdict = bool(form[0]), bool(form[1]), bool(form[2]), form[3]
    out.sums = [sm.raw[96 * b:96 * b + 96] for b in range(n)]
    out.rho = [sum(rho[4 * b + j] << (32 * j) for j in range(4)) for b in range(n)]
    out.fold, out.n_probes = fold.raw, npr.value
    out.probes = [(pr[3 * q], pr[3 * q + 1], ps.raw[96 * q:96 * q + 96], bool(pr[3 * q + 2])) for q in range(min(npr.value, max_probes))]
    out.digests = [dig.raw[32 * b:32 * b + 32] for b in range(n)]
    out.leaves = [leaves.raw[32 * k:32 * k + 32] for k in range(n * N)]
    return rc, out


FIELDS = ("verified", "status", "small", "folded", "searched", "fold_verdict", "leaves", "digests", "sums", "rho", "fold", "n_probes", "probes")


@pytest.mark.parametrize("n", [7, 2])
def test_the_tap_equals_the_tap_of_the_expanded_pass(ctx, pool, n):
    good, cells_of = pool
    if n == 7:
        items = [good[0], wrong_of(good, 1), good[2], good[3], good[1], wrong_of(good, 0, 127), good[0]]
        verdicts = [True, False, True, True, True, False, True]
    else:
        items, verdicts = [good[2], good[3]], [True, True]
    problems = [BC.expand(it, cells_of[it[0]]) for it in items]
    rc, want = TL.many_sums(ctx, problems, "device", LEAF)
    assert rc == 0 and want.verified == verdicts and want.status == [0] * n
    assert (want.small, want.folded, want.searched) == ((False, True, True) if n == 7 else (True, False, False))
    key = ("leaves", n)
    if key not in _cache:
        _cache[key] = (M.pass_leaves(problems, [True] * n), M.pass_digests(problems, [True] * n))
    for where in ("host", "device"):
        rc, got = sums(ctx, items, where)
        assert rc == 0, where
        for field in FIELDS:
            assert getattr(got, field) == getattr(want, field), (where, field)
        assert got.leaves == _cache[key][0] and got.digests == _cache[key][1], where
        assert run(ctx, items, where) == (got.verified, got.status)  # the public call says the same
    if n == 7:
        assert want.n_probes > 0 and want.fold_verdict == 0


def test_the_hook_serves_one_pass_only_and_rejects_missing_buffers(ctx, pool):
    good, _ = pool
    rc, _ = sums(ctx, [good[i % 4] for i in range(192)], "host")
    assert rc == 3
    lib = kzg.load_library()
    assert lib.eth_kzg_amd_test_verify_blob_cell_proofs_sums(None, 1, 0, *([None] * 11), 0, None, None, None) == 3
    assert lib.eth_kzg_amd_test_blob_extension(None, 1, None, None, None) == 3


# ---- 5. cuts ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_200_items_over_four_blobs_and_the_first_cut(ctx, pool, where):
    good, _ = pool
    n, first_cut = 200, BC.parts(200)[1]
    assert BC.parts(n) == [0, 67, 134, 200] and n >= BC.MIN_PROBLEMS and n * N >= BC.MIN_CELLS
    wrong = [0, first_cut - 1, first_cut, 199]
    items = [good[i % 4] for i in range(n)]  # the same four objects: the host form's blob pointers alias four buffers
    for i in wrong:
        items[i] = wrong_of(good, i % 4, k=(i * 37) % N)
    ver, st = run(ctx, items, where)
    assert st == [0] * n and [i for i in range(n) if not ver[i]] == wrong


# ---- 6. device form details --------------------------------------------------------------------------------------------------------------------
def test_device_arrays_at_odd_offsets_and_blobs_written_on_the_callers_stream(ctx, pool):
    import torch
    items = [s[0] for s in _shapes(pool).values()]
    want = _cache.get("shapes") or expect_expanded(ctx, items, pool[1])
    d = DeviceItems(items, shift=13)
    assert d.ptrs[1] % 2 == 1 and d.ptrs[2] % 2 == 1 and d.ptrs[0] % 4 == 0 and d.ptrs[0] % 16 != 0
    assert d.call(ctx) == want
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # something in front of the writes, so that they have not happened when the call is made
        a = torch.randn(4096, 4096, device="cuda")
        for _ in range(8):
            a = a @ a
            a = a / a.abs().max()
    d2 = DeviceItems(items, shift=13, stream=s)
    assert d2.call(ctx, stream=s.cuda_stream) == want
    torch.cuda.synchronize()


def test_a_host_pointer_or_a_mix_is_an_error(ctx, pool):
    items = [pool[0][0]] * 2
    d = DeviceItems(items)
    cols = [b"".join(it[0] for it in items), b"".join(it[1] for it in items), b"".join(p for it in items for p in it[2])]
    host = [np.frombuffer(c, dtype=np.uint8).copy() for c in cols]
    for holes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2)):
        ptrs = list(d.ptrs)
        for h in holes:
            ptrs[h] = host[h].ctypes.data
        with pytest.raises(kzg.KzgError, match="InvalidInput"):
            ctx.verify_blob_cell_proofs_many_device(2, *ptrs)


# ---- 7. a device list ---------------------------------------------------------------------------------------------------------------------------
def test_device_list_0_0(ctx, pool):
    good, _ = pool
    items = [good[0], wrong_of(good, 1), (BC.with_element(good[2][0], 7, R), good[2][1], good[2][2]), good[3], (good[1][0], INF, good[1][2])]
    want = ([True, False, False, True, False], [0, 0, 1, 0, 0])
    c2 = TL._ctx(devices=[0, 0], ETH_KZG_AMD_HOST_THREADS=str(MANY_HOST_THREADS))
    try:
        assert c2.verify_blob_cell_proofs_many(items) == ctx.verify_blob_cell_proofs_many(items) == want
        assert DeviceItems(items).call(c2) == want
    finally:
        c2.close()


# ---- 8. no big lock -------------------------------------------------------------------------------------------------------------------------------
def test_four_threads_next_to_the_prover(ctx, pool):
    good, _ = pool
    batches = []
    for t in range(4):
        items = [good[(i + t) % 4] for i in range(6)]
        items[t] = wrong_of(good, (2 * t) % 4, k=t)
        items[5 - t % 2] = (items[5 - t % 2][0], off_subgroup_point(), items[5 - t % 2][2])
        batches.append((items, ctx.verify_blob_cell_proofs_many(items)))  # the serial results
    assert all(w[1].count(2) == 1 and w[0].count(False) == 2 for _, w in batches)
    blob = synth.seeded_blob(1)
    serial = ctx.compute_cells_and_kzg_proofs(blob)
    errors = []

    def many(t):
        try:
            for rnd in range(3):
                where = "host" if (t + rnd) % 2 == 0 else "device"
                if run(ctx, batches[t][0], where) != batches[t][1]:
                    errors.append(("many", t, rnd, where))
        except Exception as e:  # noqa: BLE001
            errors.append(("many", t, repr(e)))

    def prover():
        try:
            for rnd in range(3):
                if ctx.compute_cells_and_kzg_proofs(blob) != serial:
                    errors.append(("prover", rnd))
        except Exception as e:  # noqa: BLE001
            errors.append(("prover", repr(e)))

    threads = [threading.Thread(target=many, args=(t,)) for t in range(4)] + [threading.Thread(target=prover)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
