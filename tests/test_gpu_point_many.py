"""eth_kzg_amd_verify_kzg_proof_many / _many_device: many verify_kzg_proof items per call, a verdict and a status for each.

Expected values come from the vectors, from the CPU oracle (one verify_kzg_proof per DISTINCT item, cached for the module) and from the
statement tests/point_many.py (hashlib, Python integers, the oracle's G1 operations); never from the library.  The hook
eth_kzg_amd_test_verify_kzg_proof_many_sums runs the public call's launches with a tap.  Host and device form unless said otherwise.

1. The 114 verify_kzg_proof vectors whose fields have the ABI's lengths in ONE call: sorted, reversed, every item doubled.
2. The order of errors: a bad point wins over a bad scalar; z = y = r - 1 is accepted.
3. n = 0, 1, 2, 63, 64, 65, 129, 1025 valid openings with wrong items planted: none, first, last, two across 63/64, every second, all.
4. Operands the equation degenerates on, alone in a pass and inside a pass of 65, pairs byte for byte.
5. Leaves, seeds, weights, full-range pairs and every probe's pair against the statement; probes consistent with the verdicts.
6. The product's own cut: P + 1 items, the wrong one at position P.
7. Device form: odd byte offsets, inputs produced on the caller's stream, a host pointer is an error.
8. A device list 0,0.
9. Four threads on one context next to the single call and the cell many-verification."""
import ctypes as C
import importlib
import os
import threading

import numpy as np
import pytest

import oracle_lib
import point_many as PM
import synth
import vectors

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu
R = PM.R
_cache = {}  # oracle answers and statements: computed once, shared by the tests, never changed


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


def expect(oracle, item):
    """(status, verdict) of one item by the CPU oracle's verify_kzg_proof, its error code as the status"""
    if item not in _cache:
        try:
            _cache[item] = (0, oracle.verify_kzg_proof(*item))
        except oracle_lib.OracleError as e:
            assert e.code in (1, 2)
            _cache[item] = (e.code, False)
    return _cache[item]


class DeviceItems:
    """the four flat arrays of a list of items in device memory, `shift` bytes into their allocations (z and y stay 4-byte aligned)"""

    def __init__(self, items, shift=0, stream=None):
        import torch
        cols = [b"".join(it[k] for it in items) or bytes(1) for k in range(4)]
        self.n, self.keep, self.ptrs = len(items), [], []
        for k, col in enumerate(cols):
            off = shift if k in (0, 3) else (shift + 3) // 4 * 4
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
        c, z, y, p = self.ptrs
        return ctx.verify_kzg_proof_many_device(self.n, c, z, y, p, stream=stream)


def run(ctx, items, where):
    if where == "host":
        return ctx.verify_kzg_proof_many(items)
    return DeviceItems(items).call(ctx)


class Sums:
    pass


def sums(ctx, items, where, forced_pass=0, max_probes=8192, max_passes=64):
    """eth_kzg_amd_test_verify_kzg_proof_many_sums -> (return code, Sums)"""
    lib = kzg.load_library()
    n = len(items)
    ver, st = (C.c_int32 * n)(), (C.c_int32 * n)()
    starts, npass = (C.c_uint64 * (max_passes + 1))(), C.c_uint64(0)
    leaves, seeds, rho = C.create_string_buffer(32 * n), C.create_string_buffer(32 * max_passes), (C.c_uint32 * (4 * n))()
    fold, fv = C.create_string_buffer(96 * max_passes), (C.c_int32 * max_passes)()
    pr, ps, npr = (C.c_int32 * (4 * max_probes))(), C.create_string_buffer(96 * max_probes), C.c_uint64(0)
    if where == "host":
        tabs = [kzg._flat_ptrs([it[k] for it in items], (48, 32, 32, 48)[k]) for k in range(4)]
        src = [t[0].ctypes.data_as(C.c_void_p) for t in tabs]
    else:
        d = DeviceItems(items)
        src = [C.c_void_p(p) for p in d.ptrs]
    rc = lib.eth_kzg_amd_test_verify_kzg_proof_many_sums(ctx.handle, n, 0 if where == "host" else 1, *src, forced_pass, ver, st, starts, max_passes,
                                                         C.byref(npass), leaves, seeds, rho, fold, fv, pr, ps, max_probes, C.byref(npr))
    out = Sums()
    out.verified, out.status = [bool(v) for v in ver], list(st)
    out.bounds = [starts[p] for p in range(npass.value + 1)] if rc == 0 else []
    out.leaves = [leaves.raw[32 * i:32 * i + 32] for i in range(n)]
    out.seeds = [seeds.raw[32 * p:32 * p + 32] for p in range(npass.value)]
    out.rho = [sum(rho[4 * i + j] << (32 * j) for j in range(4)) for i in range(n)]
    out.fold = [fold.raw[96 * p:96 * p + 96] for p in range(npass.value)]
    out.fold_verdict = [fv[p] for p in range(npass.value)]
    out.n_probes = npr.value
    out.probes = [(pr[4 * q], pr[4 * q + 1], pr[4 * q + 2], bool(pr[4 * q + 3]), ps.raw[96 * q:96 * q + 96]) for q in range(min(npr.value, max_probes))]
    return rc, out


def check_against_statement(got, items, want, pass_size=PM.PASS, tag=""):
    """everything the hook hands out against the statement; want[i] = (status, verdict)"""
    statuses, verdicts = [w[0] for w in want], [w[1] for w in want]
    bounds, passes = PM.call_statement(items, statuses, pass_size)
    assert got.bounds == bounds, (tag, got.bounds)
    assert got.status == statuses, (tag, [i for i in range(len(items)) if got.status[i] != statuses[i]][:20])
    assert got.verified == verdicts, (tag, [i for i in range(len(items)) if got.verified[i] != verdicts[i]][:20])
    for p, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
        s = passes[p]
        assert got.leaves[lo:hi] == s.leaves, (tag, p, [i for i in range(hi - lo) if got.leaves[lo + i] != s.leaves[i]][:20])
        assert got.seeds[p] == s.seed, (tag, p)
        assert got.rho[lo:hi] == s.rho, (tag, p, [i for i in range(hi - lo) if got.rho[lo + i] != s.rho[i]][:20])
        full = s.pair(0, hi - lo)
        assert got.fold[p] == full, (tag, p, got.fold[p][:48] == full[:48], got.fold[p][48:] == full[48:])
        all_valid = all(verdicts[i] for i in range(lo, hi) if statuses[i] == 0)
        assert got.fold_verdict[p] == (1 if all_valid else 0), (tag, p)
        mine = [q for q in got.probes if q[0] == p]
        assert bool(mine) == (not all_valid), (tag, p, len(mine))  # no search in a pass of valid items, one in every other
        for _, plo, phi, passed, pair in mine:
            assert 0 <= plo < phi <= hi - lo, (tag, p, plo, phi)
            assert passed == all(verdicts[lo + i] for i in range(plo, phi) if statuses[lo + i] == 0), (tag, p, plo, phi, passed)
            assert pair == s.pair(plo, phi), (tag, p, plo, phi, pair[:48] == s.pair(plo, phi)[:48], pair[48:] == s.pair(plo, phi)[48:])
        # every wrong item was pinned down by a probe of its own, every live valid one lies in a probe that passed (or in a pass that did)
        single_fail = {plo for _, plo, phi, passed, _ in mine if phi - plo == 1 and not passed}
        assert single_fail == {i - lo for i in range(lo, hi) if statuses[i] == 0 and not verdicts[i]}, (tag, p)
        if not all_valid:
            cleared = set()
            for _, plo, phi, passed, _ in mine:
                if passed:
                    cleared |= set(range(plo, phi))
            assert {i - lo for i in range(lo, hi) if statuses[i] == 0 and verdicts[i]} <= cleared, (tag, p)
    assert got.n_probes == len(got.probes), tag


# ---- material: valid openings of a few seeded blobs, from the library's prover, each confirmed by the oracle -----------------------------------
@pytest.fixture(scope="module")
def pool(ctx, oracle):
    """six distinct valid items (three blobs, two points each) and, per item, two wrong ones: y changed, the proof swapped"""
    zs = synth.seeded_scalars(2, b"point-many:z")
    good = []
    for b in range(3):
        blob = synth.seeded_blob(b)
        comm = ctx.blob_to_kzg_commitment(blob)
        for zb in zs:
            proof, y = ctx.compute_kzg_proof(blob, zb)
            good.append((comm, zb, y, proof))
    assert len(set(good)) == 6
    wrong_y = [(c, z, PM.fr_be(int.from_bytes(y, "big") + 1), p) for c, z, y, p in good]
    wrong_p = [(c, z, y, good[(i + 1) % 6][3]) for i, (c, z, y, p) in enumerate(good)]
    for it in good:
        assert expect(oracle, it) == (0, True)
    for it in wrong_y + wrong_p:
        assert expect(oracle, it) == (0, False)
    return good, wrong_y, wrong_p


# ---- 1. the vectors in one call -------------------------------------------------------------------------------------------------------------
def _vector_items(oracle):
    if "vectors" not in _cache:
        items, want, skipped = [], [], 0
        for name, case in sorted(vectors.load("verify_kzg_proof").items()):
            i = case["input"]
            it = (i["commitment"], i["z"], i["y"], i["proof"])
            if [len(f) for f in it] != [48, 32, 32, 48]:
                skipped += 1
                assert case["output"] is None, name
                continue
            st, v = expect(oracle, it)
            assert (None if st else v) == case["output"], name  # the oracle agrees with the vector
            items.append(it)
            want.append((st, v))
        assert len(items) == 114 and skipped == 8
        assert [sum(1 for w in want if w == k) for k in ((0, True), (0, False), (1, False), (2, False))] == [54, 48, 8, 4]
        _cache["vectors"] = (items, want)
    return _cache["vectors"]


@pytest.mark.parametrize("where", ["host", "device"])
def test_vectors_in_one_call(ctx, oracle, where):
    items, want = _vector_items(oracle)
    for tag, order in (("sorted", list(range(114))), ("reversed", list(range(113, -1, -1))), ("doubled", [i // 2 for i in range(228)])):
        ver, st = run(ctx, [items[i] for i in order], where)
        assert st == [want[i][0] for i in order], (tag, [k for k, i in enumerate(order) if st[k] != want[i][0]])
        assert ver == [want[i][1] for i in order], (tag, [k for k, i in enumerate(order) if ver[k] != want[i][1]])


# ---- 2. order of errors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_order_of_errors(ctx, oracle, pool, where):
    shapes = PM.error_order_items(pool[0][0])
    assert [s for _, s in shapes.values()] == [2, 2, 1, 1, 0]
    items = [it for it, _ in shapes.values()]
    want = [expect(oracle, it) for it in items]
    assert [w[0] for w in want] == [s for _, s in shapes.values()]  # the oracle's order of checks is the reference's
    ver, st = run(ctx, items, where)
    assert st == [w[0] for w in want] and ver == [w[1] for w in want], (st, ver)
    for it, w in zip(items, want):  # and each alone
        assert run(ctx, [it], where) == ([w[1]], [w[0]])


# ---- 3. sizes and places -------------------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 2, 63, 64, 65, 129, 1025]
PATTERNS = {
    "none": lambda n: [],
    "first": lambda n: [0],
    "last": lambda n: [n - 1],
    "across-63-64": lambda n: [63, 64],
    "every-second": lambda n: list(range(0, n, 2)),
    "all": lambda n: list(range(n)),
}


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_places(ctx, pool, n, where):
    good, wrong_y, wrong_p = pool
    if n == 0:
        assert ctx.verify_kzg_proof_many([]) == ([], [])
        assert ctx.verify_kzg_proof_many_device(0, 0, 0, 0, 0) == ([], [])
        return
    ran = 0
    for name, places in PATTERNS.items():
        wrong = sorted(set(places(n)))
        if any(not 0 <= i < n for i in wrong):
            continue  # the pattern needs more items
        items = [good[i % 6] for i in range(n)]
        for k, i in enumerate(wrong):
            items[i] = (wrong_y if k % 2 == 0 else wrong_p)[i % 6]
        ver, st = run(ctx, items, where)
        assert st == [0] * n, (name, [i for i in range(n) if st[i]][:20])
        assert [i for i in range(n) if not ver[i]] == wrong, (name, n)
        ran += 1
    assert ran == (6 if n >= 65 else 5)


# ---- 4. operands the equation degenerates on ------------------------------------------------------------------------------------------------------
def _degenerate(oracle):
    """{name: (item, valid)}; the openings come from the oracle's prover"""
    if "degenerate" not in _cache:
        out = {k: (it, k in ("zero-polynomial", "constant-polynomial")) for k, it in PM.degenerate_items().items()}
        blob = synth.seeded_blob(7)
        comm = oracle.blob_to_kzg_commitment(blob)
        w4096 = pow(7, (R - 1) // 4096, R)
        for name, z in (("z=0", 0), ("z-in-domain", pow(w4096, 1234, R))):
            proof, y = oracle.compute_kzg_proof(blob, PM.fr_be(z))
            out[name] = ((comm, PM.fr_be(z), y, proof), True)
        # an opening with y = 0: p(X) = X - z0, in evaluation form over the bit-reversed domain
        z0 = int.from_bytes(b"point-many:root".ljust(31, b"\0"), "big") % R
        brp = lambda v: int(format(v, "012b")[::-1], 2)  # noqa: E731
        lin = b"".join(PM.fr_be(pow(w4096, brp(i), R) - z0) for i in range(4096))
        proof, y = oracle.compute_kzg_proof(lin, PM.fr_be(z0))
        assert y == bytes(32)
        out["y=0"] = ((oracle.blob_to_kzg_commitment(lin), PM.fr_be(z0), y, proof), True)
        assert set(out) == {"zero-polynomial", "constant-polynomial", "z=0", "y=0", "z-in-domain", "doubling", "cancels", "equals-yG"}
        for name, (it, valid) in out.items():
            assert expect(oracle, it) == (0, valid), name  # the oracle gives each verdict
        _cache["degenerate"] = out
    return _cache["degenerate"]


DEGENERATE = ["zero-polynomial", "constant-polynomial", "z=0", "y=0", "z-in-domain", "doubling", "cancels", "equals-yG", "thrice"]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_operands(ctx, oracle, pool, name, where):
    deg = _degenerate(oracle)
    mine = [deg["z=0"][0]] * 3 if name == "thrice" else [deg[name][0]]
    around = [pool[0][i % 6] for i in range(65 - len(mine))]
    for tag, items in (("alone", mine), ("in-65", around[:37] + mine + around[37:])):
        assert len(items) in (1, 3, 65)
        want = [expect(oracle, it) for it in items]
        rc, got = sums(ctx, items, where)
        assert rc == 0
        check_against_statement(got, items, want, tag="%s %s %s" % (name, tag, where))


# ---- 5. bytes ---------------------------------------------------------------------------------------------------------------------------------------
def _byte_cases(oracle, pool):
    good, wrong_y, wrong_p = pool
    deg = _degenerate(oracle)
    valid200 = [good[i % 6] for i in range(200)]
    one_wrong = list(valid200)
    one_wrong[137] = wrong_p[137 % 6]
    mixed = [deg[k][0] for k in sorted(deg)] + [it for it, _ in PM.error_order_items(good[0]).values()]
    mixed = (mixed + valid200)[:65]
    cut = list(valid200)
    cut[95], cut[96], cut[199] = wrong_y[95 % 6], wrong_p[96 % 6], wrong_y[199 % 6]
    return {"all-valid-200": (valid200, 0), "one-wrong-of-200": (one_wrong, 0), "degenerate-65": (mixed, 0), "three-passes-of-96": (cut, 96)}


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", ["all-valid-200", "one-wrong-of-200", "degenerate-65", "three-passes-of-96"])
def test_bytes_against_the_statement(ctx, oracle, pool, case, where):
    items, forced = _byte_cases(oracle, pool)[case]
    want = [expect(oracle, it) for it in items]
    rc, got = sums(ctx, items, where, forced_pass=forced)
    assert rc == 0
    if forced:
        assert got.bounds == [0, 96, 192, 200]
    check_against_statement(got, items, want, pass_size=forced or PM.PASS, tag="%s %s" % (case, where))
    assert (got.n_probes == 0) == (case == "all-valid-200")
    ver, st = run(ctx, items, where)  # and the public call says the same
    assert (ver, st) == (got.verified, got.status)


# ---- 6. the product's own cut -------------------------------------------------------------------------------------------------------------------------
def test_the_products_own_cut(ctx, pool):
    good, wrong_y, _ = pool
    n = PM.PASS + 1
    items = [good[0]] * PM.PASS + [wrong_y[0]]
    for where in ("host", "device"):
        ver, st = run(ctx, items, where)
        assert st == [0] * n and [i for i in range(n) if not ver[i]] == [PM.PASS], where
    rc, got = sums(ctx, items, "host", max_probes=16)
    assert rc == 0 and got.bounds == [0, PM.PASS, n]
    assert got.fold_verdict == [1, 0] and [i for i in range(n) if not got.verified[i]] == [PM.PASS]
    assert [(q[0], q[1], q[2], q[3]) for q in got.probes] == [(1, 0, 1, False)]


# ---- 7. device form details -----------------------------------------------------------------------------------------------------------------------------
def test_device_arrays_at_odd_offsets_and_written_on_the_callers_stream(ctx, oracle):
    import torch
    items, want = _vector_items(oracle)
    d = DeviceItems(items, shift=13)
    assert d.ptrs[0] % 2 == 1 and d.ptrs[3] % 2 == 1 and d.ptrs[1] % 4 == 0 and d.ptrs[2] % 4 == 0
    assert d.call(ctx) == ([w[1] for w in want], [w[0] for w in want])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # something in front of the writes, so that they have not happened when the call is made
        a = torch.randn(4096, 4096, device="cuda")
        for _ in range(8):
            a = a @ a
            a = a / a.abs().max()
    d2 = DeviceItems(items, shift=13, stream=s)
    assert d2.call(ctx, stream=s.cuda_stream) == ([w[1] for w in want], [w[0] for w in want])
    torch.cuda.synchronize()


def test_a_host_pointer_is_an_error(ctx, pool):
    d = DeviceItems([pool[0][0]] * 3)
    host = np.frombuffer(pool[0][0][0] * 3, dtype=np.uint8).copy()
    for hole in range(4):
        ptrs = list(d.ptrs)
        ptrs[hole] = host.ctypes.data
        with pytest.raises(kzg.KzgError, match="InvalidInput"):
            ctx.verify_kzg_proof_many_device(3, *ptrs)


# ---- 8. a device list ---------------------------------------------------------------------------------------------------------------------------------------
def test_device_list_0_0(oracle):
    items, want = _vector_items(oracle)
    c2 = _ctx(devices=[0, 0])
    try:
        for where in ("host", "device"):
            assert run(c2, items, where) == ([w[1] for w in want], [w[0] for w in want]), where
    finally:
        c2.close()


# ---- 9. threads ------------------------------------------------------------------------------------------------------------------------------------------------
def test_four_threads_next_to_the_single_call_and_the_cell_many_verification(ctx, oracle, pool):
    good, wrong_y, wrong_p = pool
    vec_items, vec_want = _vector_items(oracle)
    batches = []
    for t in range(4):
        items = [good[(i + t) % 6] for i in range(300 + 17 * t)]
        for i in range(t, len(items), 41 + t):
            items[i] = wrong_y[(i + t) % 6]
        batches.append((items + vec_items[:20 * t], None))
    batches = [(items, ([expect(oracle, it)[1] for it in items], [expect(oracle, it)[0] for it in items])) for items, _ in batches]
    blob = synth.seeded_blob(1)
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch([blob])
    comm = ctx.blob_to_kzg_commitment(blob)
    problem = ([comm] * 128, list(range(128)), cells[0], proofs[0])
    bad = ([comm] * 128, list(range(128)), cells[0], proofs[0][1:] + proofs[0][:1])
    errors = []

    def many(t):
        try:
            for rnd in range(3):
                where = "host" if (t + rnd) % 2 == 0 else "device"
                got = run(ctx, batches[t][0], where)
                if got != batches[t][1]:
                    errors.append(("many", t, rnd, where))
        except Exception as e:  # noqa: BLE001
            errors.append(("many", t, repr(e)))

    def others():
        try:
            for rnd in range(3):
                for it in (good[rnd], wrong_p[rnd]):
                    if ctx.verify_kzg_proof(*it) != expect(oracle, it)[1]:
                        errors.append(("single", rnd))
                if ctx.verify_cell_kzg_proof_batch_many([problem, bad, problem]) != ([True, False, True], [0, 0, 0]):
                    errors.append(("cells", rnd))
        except Exception as e:  # noqa: BLE001
            errors.append(("others", repr(e)))

    threads = [threading.Thread(target=many, args=(t,)) for t in range(4)] + [threading.Thread(target=others)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
