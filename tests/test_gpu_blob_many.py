"""eth_kzg_amd_verify_blob_kzg_proof_many / _many_device: many verify_blob_kzg_proof items per call, a verdict and a status for each.

Expected values come from the vectors, from eth_kzg_verify_blob_kzg_proof on the item alone (the single call this one must agree with; one
call per DISTINCT item, cached for the module), from the CPU oracle and from the statement (tests/blob_many.py over tests/point_many.py:
hashlib, Python integers, the oracle's G1 operations).  The hook eth_kzg_amd_test_verify_blob_kzg_proof_many_sums runs the public call's
launches with a tap.  Host and device form unless said otherwise.

1. The reference vectors: the 23 well-formed verify_blob_kzg_proof cases in ONE call; the 15 well-formed batch cases flattened into items.
2. The order of errors and degenerate items, item by item against the single call.
3. The statement byte for byte: z, y, leaves, seeds, weights, full-range pairs, fold verdicts and every probe; n = 7 in passes of 3, n = 1.
4. The product's pass size: 300 items over 4 blobs, wrong proofs at 0, either side of the first cut and 299; nine wrong items.
5. Device form: odd byte offsets, a host pointer or a mix is an error, blobs written on the caller's stream are seen.
6. A device list 0,0.
7. Four threads next to compute_cells_and_kzg_proofs on one context: no big lock, same results."""
import ctypes as C
import importlib
import os
import threading

import numpy as np
import pytest

import blob_many as BM
import oracle_lib
import point_many as PM
import synth
import vectors
from verify_transcript import off_subgroup_point

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu
R = BM.R
INF = BM.INF
_cache = {}  # the single call's answers and the material: computed once, shared by the tests, never changed


def _ctx(devices=None):
    import torch
    torch.cuda.init()
    saved = os.environ.get("ETH_KZG_AMD_TABLE_GB")
    os.environ["ETH_KZG_AMD_TABLE_GB"] = "3"  # the start tables: results never depend on the table
    try:
        return kzg.DASContext(use_precomp=True, devices=devices)
    finally:
        if saved is None:
            os.environ.pop("ETH_KZG_AMD_TABLE_GB", None)
        else:
            os.environ["ETH_KZG_AMD_TABLE_GB"] = saved


@pytest.fixture(scope="module")
def ctx():
    c = _ctx()
    yield c
    c.close()


def single(ctx, item):
    """(status, verdict) of one item by eth_kzg_verify_blob_kzg_proof, its error class as the status"""
    if item not in _cache:
        try:
            _cache[item] = (0, ctx.verify_blob_kzg_proof(*item))
        except kzg.KzgError as e:
            _cache[item] = ({"Serialization(CouldNotDeserializeScalar)": 1, "Serialization(CouldNotDeserializeG1Point)": 2}[str(e)], False)
    return _cache[item]


class DeviceItems:
    """the three flat arrays of a list of items in device memory; commitments and proofs `shift` bytes into their allocations, the blobs
    at the next multiple of four"""

    def __init__(self, items, shift=0, stream=None):
        import torch
        cols = [b"".join(it[k] for it in items) or bytes(1) for k in range(3)]
        self.n, self.keep, self.ptrs = len(items), [], []
        for k, col in enumerate(cols):
            off = ((shift + 3) // 4 * 4 + 4 if shift else 0) if k == 0 else shift  # (13 -> 20: a multiple of 4 and not of 16)
            a = torch.from_numpy(np.frombuffer(col, dtype=np.uint8).copy())
            if stream is None:
                d = torch.empty(off + len(col), dtype=torch.uint8, device="cuda")
                d[off:].copy_(a)
            else:  # written by a kernel queued on the caller's stream: the call must wait for it
                with torch.cuda.stream(stream):
                    staged = a.pin_memory().to("cuda", non_blocking=True)
                    d = torch.zeros(off + len(col), dtype=torch.uint8, device="cuda")
                    d[off:] = staged ^ 0  # an elementwise kernel, not a copy engine
                self.keep.append(staged)
            self.keep.append(d)
            self.ptrs.append(d.data_ptr() + off)
        if stream is None:
            torch.cuda.synchronize()

    def call(self, ctx, stream=None):
        return ctx.verify_blob_kzg_proof_many_device(self.n, *self.ptrs, stream=stream)


def run(ctx, items, where):
    if where == "host":
        return ctx.verify_blob_kzg_proof_many(items)
    return DeviceItems(items).call(ctx)


def expect_single(ctx, items):
    want = [single(ctx, it) for it in items]
    return [w[1] for w in want], [w[0] for w in want]


# ---- material ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(ctx, oracle):
    """four distinct valid items from the oracle's prover, and what the single call says of them"""
    good = []
    for b in range(4):
        blob = synth.seeded_blob(40 + b)
        comm = oracle.blob_to_kzg_commitment(blob)
        good.append((blob, comm, oracle.compute_blob_kzg_proof(blob, comm)))
    for it in good:
        assert single(ctx, it) == (0, True)
    return good


def wrong_of(good, i):
    """item i with another blob's proof"""
    return (good[i][0], good[i][1], good[(i + 1) % len(good)][2])


# ---- 1. the reference vectors --------------------------------------------------------------------------------------------------------------
def _well_formed(blobs, comms, proofs):
    return len(blobs) == len(comms) == len(proofs) and all(len(b) == BM.BLOB_BYTES for b in blobs) and all(len(x) == 48 for x in comms + proofs)


@pytest.mark.parametrize("where", ["host", "device"])
def test_single_vectors_in_one_call(ctx, where):
    items, outputs, skipped = [], [], 0
    for name, case in sorted(vectors.load("verify_blob_kzg_proof").items()):
        i = case["input"]
        if not _well_formed([i["blob"]], [i["commitment"]], [i["proof"]]):
            skipped += 1
            assert case["output"] is None, name
            continue
        items.append((i["blob"], i["commitment"], i["proof"]))
        outputs.append(case["output"])
    assert len(items) == 23 and skipped == 6
    ver, st = run(ctx, items, where)
    for k, out in enumerate(outputs):
        if out is None:
            assert st[k] != 0 and ver[k] is False, k
        else:
            assert (st[k], ver[k]) == (0, out), k
        assert (st[k], ver[k]) == single(ctx, items[k]), k
    assert None in outputs and True in outputs and False in outputs


@pytest.mark.parametrize("where", ["host", "device"])
def test_batch_vectors_flattened_into_items(ctx, where):
    seen = skipped = 0
    for name, case in sorted(vectors.load("verify_blob_kzg_proof_batch").items()):
        i = case["input"]
        if not _well_formed(i["blobs"], i["commitments"], i["proofs"]):
            skipped += 1
            continue
        seen += 1
        items = list(zip(i["blobs"], i["commitments"], i["proofs"]))
        ver, st = run(ctx, items, where)
        if case["output"] is True:
            assert st == [0] * len(items) and ver == [True] * len(items), name
        elif case["output"] is False:
            assert not any(st) and False in ver, name
        else:
            assert any(st), name
        assert (ver, st) == expect_single(ctx, items), name
    assert (seen, skipped) == (15, 9)


# ---- 2. order of errors, degenerate items ----------------------------------------------------------------------------------------------------
def _shapes(pool):
    a, b = pool[0], pool[1]
    off_curve = next(c for c in (bytes([0x80]) + x.to_bytes(47, "big") for x in range(1, 64)) if oracle_lib.g1_validate(c, False) != 0)
    off = off_subgroup_point()
    assert oracle_lib.g1_validate(off, False) == 0 and oracle_lib.g1_validate(off, True) != 0
    non_canonical = b"\xc0" + bytes(46) + b"\x01"  # the identity's flags over a non-zero field
    bad_blob = BM.with_element(a[0], 4095, R)
    return {
        "valid": (a, 0),
        "wrong-proof": ((a[0], a[1], b[2]), 0),
        "identity-proof-for-a-non-constant-blob": ((a[0], a[1], INF), 0),
        "commitment-off-the-curve": ((a[0], off_curve, a[2]), 2),
        "proof-outside-the-subgroup": ((a[0], a[1], off), 2),
        "non-canonical-encoding": ((a[0], non_canonical, a[2]), 2),
        "blob-bad-and-commitment-bad": ((bad_blob, off_curve, a[2]), 1),
        "blob-bad-everything-else-valid": ((bad_blob, a[1], a[2]), 1),
        "zero-blob-with-two-identities": ((bytes(BM.BLOB_BYTES), INF, INF), 0),
        "valid-again": (a, 0),
        "another-valid": (b, 0),
    }


@pytest.mark.parametrize("where", ["host", "device"])
def test_order_of_errors_and_degenerate_items(ctx, pool, where):
    shapes = _shapes(pool)
    items = [it for it, _ in shapes.values()]
    assert [BM.item_status(it) for it in items] == [s for _, s in shapes.values()]  # the statement's order is the issue's
    want = expect_single(ctx, items)
    assert want[1] == [s for _, s in shapes.values()]
    assert want[0] == [k in ("valid", "zero-blob-with-two-identities", "valid-again", "another-valid") for k in shapes]
    assert run(ctx, items, where) == want
    for it in items[1:9]:  # and each alone
        assert run(ctx, [it], where) == expect_single(ctx, [it])
    assert ctx.verify_blob_kzg_proof_many([]) == ([], []) and ctx.verify_blob_kzg_proof_many_device(0, 0, 0, 0) == ([], [])


# ---- 3. the statement, byte for byte ---------------------------------------------------------------------------------------------------------
class Sums:
    pass


def sums(ctx, items, where, forced_pass=0, max_probes=512, max_passes=16):
    """eth_kzg_amd_test_verify_blob_kzg_proof_many_sums -> (return code, Sums)"""
    lib = kzg.load_library()
    n = len(items)
    ver, st = (C.c_int32 * n)(), (C.c_int32 * n)()
    starts, npass = (C.c_uint64 * (max_passes + 1))(), C.c_uint64(0)
    leaves, seeds, rho = C.create_string_buffer(32 * n), C.create_string_buffer(32 * max_passes), (C.c_uint32 * (4 * n))()
    fold, fv = C.create_string_buffer(96 * max_passes), (C.c_int32 * max_passes)()
    pr, ps, npr = (C.c_int32 * (4 * max_probes))(), C.create_string_buffer(96 * max_probes), C.c_uint64(0)
    zs, ys = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n)
    if where == "host":
        tabs = [kzg._alias_ptrs([it[0] for it in items])] + [kzg._flat_ptrs([it[k] for it in items], 48) for k in (1, 2)]
        src = [t[0].ctypes.data_as(C.c_void_p) for t in tabs]
    else:
        d = DeviceItems(items)
        src = [C.c_void_p(p) for p in d.ptrs]
    rc = lib.eth_kzg_amd_test_verify_blob_kzg_proof_many_sums(ctx.handle, n, 0 if where == "host" else 1, *src, forced_pass, ver, st, starts, max_passes,
                                                              C.byref(npass), leaves, seeds, rho, fold, fv, pr, ps, max_probes, C.byref(npr), zs, ys)
    out = Sums()
    out.verified, out.status = [bool(v) for v in ver], list(st)
    out.bounds = [starts[p] for p in range(npass.value + 1)] if rc == 0 else []
    cut = lambda buf, size, count: [buf.raw[size * i:size * i + size] for i in range(count)]  # noqa: E731
    out.leaves, out.zs, out.ys = cut(leaves, 32, n), cut(zs, 32, n), cut(ys, 32, n)
    out.seeds, out.fold = cut(seeds, 32, npass.value), cut(fold, 96, npass.value)
    out.rho = [sum(rho[4 * i + j] << (32 * j) for j in range(4)) for i in range(n)]
    out.fold_verdict = [fv[p] for p in range(npass.value)]
    out.n_probes = npr.value
    out.probes = [(pr[4 * q], pr[4 * q + 1], pr[4 * q + 2], bool(pr[4 * q + 3]), ps.raw[96 * q:96 * q + 96]) for q in range(min(npr.value, max_probes))]
    return rc, out


def check_against_statement(got, items, statuses, verdicts, ys, pass_size, tag):
    bounds, passes, pts = BM.call_statement(items, statuses, ys, pass_size)
    assert got.bounds == bounds, (tag, got.bounds)
    assert (got.status, got.verified) == (statuses, verdicts), (tag, got.status, got.verified)
    assert got.zs == [p[1] for p in pts], (tag, [i for i in range(len(items)) if got.zs[i] != pts[i][1]])
    assert got.ys == [p[2] for p in pts], (tag, [i for i in range(len(items)) if got.ys[i] != pts[i][2]])
    for p, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
        s = passes[p]
        assert got.leaves[lo:hi] == s.leaves, (tag, p)
        assert got.seeds[p] == s.seed, (tag, p)
        assert got.rho[lo:hi] == s.rho, (tag, p)
        full = s.pair(0, hi - lo)
        assert got.fold[p] == full, (tag, p, got.fold[p][:48] == full[:48], got.fold[p][48:] == full[48:])
        all_valid = all(verdicts[i] for i in range(lo, hi) if statuses[i] == 0)
        assert got.fold_verdict[p] == (1 if all_valid else 0), (tag, p)
        mine = [q for q in got.probes if q[0] == p]
        assert bool(mine) == (not all_valid), (tag, p, len(mine))
        for _, plo, phi, passed, pair in mine:
            assert 0 <= plo < phi <= hi - lo, (tag, p, plo, phi)
            assert passed == all(verdicts[lo + i] for i in range(plo, phi) if statuses[lo + i] == 0), (tag, p, plo, phi)
            assert pair == s.pair(plo, phi), (tag, p, plo, phi)
        single_fail = {plo for _, plo, phi, passed, _ in mine if phi - plo == 1 and not passed}
        assert single_fail == {i - lo for i in range(lo, hi) if statuses[i] == 0 and not verdicts[i]}, (tag, p)
    assert got.n_probes == len(got.probes), tag


def _statement_items(pool, oracle):
    """n = 7: every status, a wrong item in two of the three passes of 3, the identity item; with y from the oracle"""
    if "statement" not in _cache:
        sh = _shapes(pool)
        names = ["valid", "wrong-proof", "blob-bad-and-commitment-bad", "commitment-off-the-curve", "another-valid",
                 "zero-blob-with-two-identities", "identity-proof-for-a-non-constant-blob"]
        items = [sh[k][0] for k in names]
        statuses = [BM.item_status(it) for it in items]
        ys = []
        for (blob, c, _), s in zip(items, statuses):
            ys.append(bytes(32) if s == 1 else oracle.compute_kzg_proof(blob, BM.fr_be(BM.blob_challenge(blob, c)))[1])
        _cache["statement"] = (items, statuses, ys)
    return _cache["statement"]


@pytest.mark.parametrize("n,forced", [(7, 3), (1, 0)])
def test_bytes_against_the_statement(ctx, oracle, pool, n, forced):
    items, statuses, ys = (v[:n] for v in _statement_items(pool, oracle))
    assert n == 1 or statuses == [0, 0, 1, 2, 0, 0, 0]
    verdicts = expect_single(ctx, items)[0]
    got = {}
    for where in ("host", "device"):
        rc, got[where] = sums(ctx, items, where, forced_pass=forced)
        assert rc == 0
        check_against_statement(got[where], items, statuses, verdicts, ys, forced or BM.PASS, "%d %s" % (n, where))
        assert run(ctx, items, where) == (got[where].verified, got[where].status)  # the public call says the same
    if n == 7:
        assert got["host"].bounds == [0, 3, 6, 7] and got["host"].fold_verdict == [0, 1, 0]
    for field in ("bounds", "status", "verified", "zs", "ys", "leaves", "seeds", "rho", "fold", "fold_verdict", "probes"):
        assert getattr(got["host"], field) == getattr(got["device"], field), field  # and the two forms agree with each other


# ---- 4. passes and search at the product's pass size -------------------------------------------------------------------------------------------
def test_300_items_over_four_blobs_and_the_first_cut(ctx, pool):
    n, wrong = 300, [0, BM.PASS - 1, BM.PASS, 299]
    assert BM.PASS == 256
    items = [pool[i % 4] for i in range(n)]  # the same four objects: the host form's pointers alias four buffers
    for i in wrong:
        items[i] = wrong_of(pool, i % 4)
        assert single(ctx, items[i]) == (0, False)
    ver, st = ctx.verify_blob_kzg_proof_many(items)
    assert st == [0] * n and [i for i in range(n) if not ver[i]] == wrong


def test_257_device_items_in_two_passes_side_by_side_behind_the_callers_stream(ctx, pool):
    """BM.PASS + 1 items in device memory: the smallest call whose two passes run side by side on two pass slots (no tap), each putting
    its slot's stream behind the caller's, on which the three arrays are still being written when the call is made"""
    import torch
    n, wrong = BM.PASS + 1, [0, BM.PASS - 1, BM.PASS]
    assert n == 257
    items = [pool[i % 4] for i in range(n)]
    for i in wrong:
        items[i] = wrong_of(pool, i % 4)
    want = expect_single(ctx, items)  # the single call on the four distinct items and the wrong ones
    assert want[1] == [0] * n and [i for i in range(n) if not want[0][i]] == wrong
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # something in front of the writes, so that they have not happened when the call is made
        a = torch.randn(4096, 4096, device="cuda")
        for _ in range(8):
            a = a @ a
            a = a / a.abs().max()
    d = DeviceItems(items, stream=s)
    ver, st = d.call(ctx, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert st == [0] * n and [i for i in range(n) if not ver[i]] == wrong
    assert (ver, st) == want


@pytest.mark.parametrize("where", ["host", "device"])
def test_nine_wrong_items(ctx, pool, where):
    items = [wrong_of(pool, i % 4) for i in range(9)]
    assert run(ctx, items, where) == ([False] * 9, [0] * 9)


# ---- 5. device form details -----------------------------------------------------------------------------------------------------------------------
def test_device_arrays_at_odd_offsets_and_blobs_written_on_the_callers_stream(ctx, pool):
    import torch
    items = [it for it, _ in _shapes(pool).values()]
    want = expect_single(ctx, items)
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
    items = [pool[0]] * 2
    d = DeviceItems(items)
    host = [np.frombuffer(b"".join(it[k] for it in items), dtype=np.uint8).copy() for k in range(3)]
    for holes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2)):
        ptrs = list(d.ptrs)
        for h in holes:
            ptrs[h] = host[h].ctypes.data
        with pytest.raises(kzg.KzgError, match="InvalidInput"):
            ctx.verify_blob_kzg_proof_many_device(2, *ptrs)


# ---- 6. a device list ---------------------------------------------------------------------------------------------------------------------------------
def test_device_list_0_0(ctx, pool):
    items = [pool[0], wrong_of(pool, 1), (BM.with_element(pool[2][0], 7, R), pool[2][1], pool[2][2]), pool[3], (pool[1][0], INF, pool[1][2])]
    want = expect_single(ctx, items)
    assert want == ([True, False, False, True, False], [0, 0, 1, 0, 0])
    c2 = _ctx(devices=[0, 0])
    try:
        assert c2.verify_blob_kzg_proof_many(items) == ctx.verify_blob_kzg_proof_many(items) == want
        assert DeviceItems(items).call(c2) == want
        one, two = sums(ctx, items, "host")[1], sums(c2, items, "host")[1]  # the hook runs on the first engine of either context
        for field in ("status", "verified", "zs", "ys", "leaves", "seeds", "rho", "fold"):
            assert getattr(one, field) == getattr(two, field), field
    finally:
        c2.close()


# ---- 7. no big lock -----------------------------------------------------------------------------------------------------------------------------------------
def test_four_threads_next_to_the_prover(ctx, pool):
    batches = []
    for t in range(4):
        items = [pool[(i + t) % 4] for i in range(8)]
        items[t] = wrong_of(pool, (2 * t) % 4)
        items[7 - t] = (items[7 - t][0], off_subgroup_point(), items[7 - t][2])
        batches.append((items, expect_single(ctx, items)))
    assert all(False in w[0] and 2 in w[1] for _, w in batches)
    blob = synth.seeded_blob(1)
    serial = ctx.compute_cells_and_kzg_proofs(blob)
    for items, want in batches:
        assert ctx.verify_blob_kzg_proof_many(items) == want  # the serial results
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
