"""The many-verification with leaf-hashed challenges and on flat arrays in HBM: eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex and
eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex.

The statement is tests/many_leaf.py (hashlib and Python integers: per problem the single flagged call's challenge, then
verify_transcript's pair, weights, fold and search plan unchanged).  The hooks eth_kzg_amd_test_verify_many_sums_ex / _device run one
pass with the taps of tests/test_verify_inputs.py's hook plus the digests the challenges were reduced from and the leaf digests.
Contexts as test_verify_inputs.py's many_ctx: small tables, two host threads.

1. Leaves and roots across wave and problem boundaries: one pass of 326 cells in problems of 1, 63, 64, 65, 2, 0, 3, 128.
2. Every form a pass takes (verify_transcript.many_cases(), in process), three ways: host flagged, device flagged, device unflagged
   (the last against the reference-transcript statement test_verify_inputs.py holds the host form to).
3. The public calls agree on a pass of every ManyProblem kind; the call-level InvalidInput cases with a NULL context.
4. Byte arrays 8 bytes into their allocations, produced by asynchronous copies on the caller's stream; a refused problem beside an
   empty one between two runs of device-to-device copies (3, 0, 2, 65, 1 cells), against the pointer-list form, byte for byte.
5. Cuts: 192 x 128 cells (three concurrent parts), 1025 x 128 + 3 cells (parts again) and 136 x 1024 cells (two chunks on one slot, with
   refused problems around the chunk boundary), one swapped-proof problem beyond the first cut; a problem of 2^24 cells is refused unread.
6. The reference's 30 verify_cell_kzg_proof_batch vectors as the problems of one call.
7. A device list 0,0: the host form sliced, the device form by owner; all four pointers are resolved.
8. Four threads on one context."""
import ctypes as C
import importlib
import os
import threading
import time

import numpy as np
import pytest

import many_leaf as M
import vectors
import verify_transcript as T

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu

LEAF = 1  # ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT
CELL_CASES = {c.name: c for c in T.cell_cases()}
MANY_PASSES = {p.name: p for p in T.many_cases()}
IN_PROCESS = [name for name in MANY_PASSES if name != "folded-ten"]  # (that one is for a process with the four-lane kernels switched off)
COOP_POINTS_MAX = 8192
WAYS = {"host-leaf": ("host", LEAF), "device-leaf": ("device", LEAF), "device-reference": ("device", 0)}
_statement = {}  # computed once, shared by the ways and the tests, never changed


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
    c = _ctx(ETH_KZG_AMD_HOST_THREADS=str(T.MANY_HOST_THREADS))
    yield c
    c.close()


@pytest.fixture(scope="module")
def material(ctx):
    blobs = T.material_blobs()
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(blobs)
    assert st == [0] * len(blobs)
    comms = [ctx.blob_to_kzg_commitment(b) for b in blobs]
    return T.Material(blobs, comms, cells, proofs, [None] * len(blobs))


class DeviceArrays:
    """the flat arrays of a list of problems in device memory; `shift` bytes into their allocations"""

    def __init__(self, problems, shift=0, stream=None):
        import torch
        self.starts, comm, idx, cells, proofs = M.flat_arrays(problems)
        host = [np.frombuffer(b"".join(comm) or bytes(1), dtype=np.uint8), np.array(idx or [0], dtype=np.uint64).view(np.uint8),
                np.frombuffer(b"".join(cells) or bytes(1), dtype=np.uint8), np.frombuffer(b"".join(proofs) or bytes(1), dtype=np.uint8)]
        self.keep, self.ptrs = [], []
        for a in host:
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

    def call(self, ctx, leaf, stream=None):
        return ctx.verify_cell_kzg_proof_batch_many_device(self.starts, *self.ptrs, stream=stream, leaf_transcript=leaf)


class ManySums:
    pass


def many_sums(ctx, problems, where, flags, max_probes=256):
    """eth_kzg_amd_test_verify_many_sums_ex (where = "host") / _device -> (return code, ManySums): what tests/many_coop_off_check.py's
    many_sums hands out, plus digests[B] and leaves[N] (32 bytes each)"""
    lib = kzg.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nb = len(problems)
    n_cells = sum(len(p[1]) for p in problems)
    ver, st, form = (C.c_int32 * nb)(), (C.c_int32 * nb)(), (C.c_int32 * 4)()
    sums, rho, fold = C.create_string_buffer(96 * nb), (C.c_uint32 * (4 * nb))(), C.create_string_buffer(96)
    pr, ps, npr = (C.c_int32 * (3 * max_probes))(), C.create_string_buffer(96 * max_probes), C.c_uint64(0)
    dig, leaves = C.create_string_buffer(32 * nb), C.create_string_buffer(32 * max(1, n_cells))
    tail = (flags, ver, st, form, sums, rho, fold, pr, ps, max_probes, C.byref(npr), dig, leaves)
    if where == "host":
        _, lens, tabs, _keep = ctx._marshal_many(problems)
        rc = lib.eth_kzg_amd_test_verify_many_sums_ex(ctx.handle, nb, vp(lens[0]), vp(tabs[0]), vp(lens[1]), vp(tabs[1]), vp(lens[2]), vp(tabs[2]),
                                                      vp(lens[3]), vp(tabs[3]), *tail)
    else:
        d = DeviceArrays(problems)
        cs = np.array(d.starts, dtype=np.uint64)
        rc = lib.eth_kzg_amd_test_verify_many_sums_device(ctx.handle, nb, vp(cs), *[C.c_void_p(p) for p in d.ptrs], *tail)
    out = ManySums()
    out.verified, out.status = [bool(v) for v in ver], list(st)
    out.small, out.folded, out.searched, out.fold_verdict = bool(form[0]), bool(form[1]), bool(form[2]), form[3]
    out.sums = [sums.raw[96 * b:96 * b + 96] for b in range(nb)]
    out.rho = [sum(rho[4 * b + j] << (32 * j) for j in range(4)) for b in range(nb)]
    out.fold, out.n_probes = fold.raw, npr.value
    out.probes = [(pr[3 * q], pr[3 * q + 1], ps.raw[96 * q:96 * q + 96], bool(pr[3 * q + 2])) for q in range(min(npr.value, max_probes))]
    out.digests = [dig.raw[32 * b:32 * b + 32] for b in range(nb)]
    out.leaves = [leaves.raw[32 * k:32 * k + 32] for k in range(n_cells)]
    return rc, out


# ---- 1. leaves and roots across wave and problem boundaries ------------------------------------------------------------------------------------
BOUNDARY_COUNTS = [1, 63, 64, 65, 2, 0, 3, 128]


def _boundary_problems(mat):
    import random
    rng = random.Random("many-leaf:boundaries")
    out = []
    for n in BOUNDARY_COUNTS:
        entries = [(rng.choice((0, 1, 2, T.B_CONST)), rng.randrange(T.N_CELLS)) for _ in range(n)]
        if n >= 2:
            entries[0], entries[-1] = (entries[0][0], 0), (entries[0][0], 127)  # a repeated commitment, the indices 0 and 127
        out.append(T.CellCase("boundary-%d" % n, entries).args(mat))
    return out


@pytest.mark.parametrize("where", ["host", "device"])
def test_leaves_and_roots_across_wave_and_problem_boundaries(ctx, material, where):
    problems = _boundary_problems(material)
    assert [len(p[1]) for p in problems] == BOUNDARY_COUNTS and sum(BOUNDARY_COUNTS) == 326 and 326 % 64 == 6
    hashed = [n > 0 for n in BOUNDARY_COUNTS]
    if "boundary" not in _statement:
        _statement["boundary"] = (M.pass_leaves(problems, hashed), M.pass_digests(problems, hashed))
    want_leaves, want_digests = _statement["boundary"]
    rc, got = many_sums(ctx, problems, where, LEAF)
    assert rc == 0
    bad = [k for k in range(326) if got.leaves[k] != want_leaves[k]]
    assert not bad, (where, bad[:20])
    assert got.digests == want_digests, (where, [b for b in range(8) if got.digests[b] != want_digests[b]])
    assert got.digests[5] == bytes(32) and got.status == [0] * 8 and got.verified == [True] * 8
    assert not got.small and got.folded and got.fold_verdict == 1


# ---- 2. every form a pass takes, three ways ----------------------------------------------------------------------------------------------------
def _pass_statement(mat, p, flags):
    """-> (digests, sums, rho, fold) of the pass under the leaf-hashed (flags) or the reference's (0) challenges"""
    key = ("pass", p.name, flags)
    if key not in _statement:
        problems = [q.args(mat) for q in p.problems]
        hashed, live = [q.hashed for q in p.problems], [q.live for q in p.problems]
        if flags:
            _statement[key] = M.pass_statement(problems, hashed, live, p.folded)
        else:
            digests = [T.cell_digest(*a) if on else bytes(32) for a, on in zip(problems, hashed)]
            sums = [T.cell_partial(*a, 0, len(a[1]), r=T.reduce_digest(d)) if on else None for a, d, on in zip(problems, digests, live)]
            rho = T.fold_weights(digests, live)
            _statement[key] = (digests, sums, rho, T.fold_pair(sums, rho, 0, len(sums)) if p.folded else None)
    return _statement[key]


def _probe_statement(p, flags, sums, rho, lo, hi):
    key = ("probe", p.name, flags, lo, hi)
    if key not in _statement:
        _statement[key] = T.fold_pair(sums, rho, lo, hi)
    return _statement[key]


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("name", IN_PROCESS)
def test_every_form_of_a_pass_equals_the_statement(ctx, material, name, way):
    where, flags = WAYS[way]
    p = MANY_PASSES[name]
    p.check(T.MANY_HOST_THREADS, COOP_POINTS_MAX)
    problems = [q.args(material) for q in p.problems]
    digests, sums, rho, fold = _pass_statement(material, p, flags)
    live, verdicts = [q.live for q in p.problems], [q.verdict for q in p.problems]
    t0 = time.perf_counter()
    rc, got = many_sums(ctx, problems, where, flags)
    print("%s %s: hook %.3f s" % (name, way, time.perf_counter() - t0))
    assert rc == 0, (name, way, rc)
    assert (got.small, got.folded, got.searched) == (p.small, p.folded, p.searched), (name, way, got.small, got.folded, got.searched)
    assert got.status == [q.status for q in p.problems], (name, way, got.status)
    assert got.verified == verdicts, (name, way, [b for b in range(len(verdicts)) if got.verified[b] != verdicts[b]])
    assert got.digests == digests, (name, way, [b for b in range(len(digests)) if got.digests[b] != digests[b]][:20])
    bad = [(b, got.sums[b][:48] == sums[b][:48], got.sums[b][48:] == sums[b][48:]) for b in range(len(problems)) if live[b] and got.sums[b] != sums[b]]
    assert not bad, "%s %s: (problem, A equal, B equal) %s" % (name, way, bad[:20])
    if p.folded:
        assert got.rho == rho, (name, way, [b for b in range(len(rho)) if got.rho[b] != rho[b]][:20])
        assert got.fold == fold, (name, way, got.fold[:48] == fold[:48], got.fold[48:] == fold[48:])
        assert got.fold_verdict == (1 if all(v for v, on in zip(verdicts, live) if on) else 0), (name, way)
    if p.searched:
        plan = T.search_plan(live, verdicts, T.MANY_HOST_THREADS)
        assert got.n_probes == len(got.probes) == len(plan), (name, way, got.n_probes)
        assert [(lo, hi, ok) for lo, hi, _, ok in got.probes] == plan, (name, way)
        bad = [(lo, hi) for lo, hi, raw, _ in got.probes if raw != _probe_statement(p, flags, sums, rho, lo, hi)]
        assert not bad, (name, way, bad)
    else:
        assert got.n_probes == 0
    if flags:
        hashed = [q.hashed for q in p.problems]
        if ("leaves", p.name) not in _statement:
            _statement[("leaves", p.name)] = M.pass_leaves(problems, hashed)
        want_leaves = _statement[("leaves", p.name)]
        bad = [k for k in range(len(want_leaves)) if got.leaves[k] != want_leaves[k]]
        assert not bad, (name, way, bad[:20])


def test_the_new_hooks_serve_one_pass_only_and_reject_missing_buffers(ctx, material):
    one = CELL_CASES["all-128-indices"].args(material)
    for where in ("host", "device"):
        rc, _ = many_sums(ctx, [one] * 192, where, LEAF)
        assert rc == 3, where
    lib = kzg.load_library()
    out = C.create_string_buffer(96)
    one64 = (C.c_uint64 * 2)(0, 1)
    i32 = (C.c_int32 * 4)()
    tail = [i32, i32, i32, out, (C.c_uint32 * 4)(), out, None, None, 0, one64, out, None]
    for missing in (0, 1, 2, 3, 4, 5, 9, 10):
        t = [None if i == missing else a for i, a in enumerate(tail)]
        assert lib.eth_kzg_amd_test_verify_many_sums_device(None, 1, one64, None, None, None, None, LEAF, *t) == 3, missing
        assert lib.eth_kzg_amd_test_verify_many_sums_ex(None, 1, one64, one64, one64, one64, one64, one64, one64, one64, LEAF, *t) == 3, missing
    assert lib.eth_kzg_amd_test_verify_many_sums_device(None, 1, one64, None, None, None, None, 2, *tail) == 3  # an unknown flag
    assert lib.eth_kzg_amd_test_verify_many_sums_device(None, 1, (C.c_uint64 * 2)(1, 1), None, None, None, None, LEAF, *tail) == 3  # cell_starts
    assert lib.eth_kzg_amd_test_verify_many_sums_device(None, 1, one64, None, None, None, None, LEAF, *tail) == 3  # cells and no arrays


# ---- 3. the public calls agree ----------------------------------------------------------------------------------------------------------------
def _kinds_pass(mat):
    """a pass that holds every ManyProblem kind (six problems: folded under two host threads)"""
    case = CELL_CASES["len-65"]
    proofs = case.args(mat)[3]
    swap = next((i, j) for i in range(65) for j in range(i + 1, 65) if proofs[i] != proofs[j])
    qs = [T.ManyProblem(CELL_CASES["len-63"]), T.ManyProblem(T.CellCase("empty", []), "empty"), T.ManyProblem(case, "swapped", swap),
          T.ManyProblem(CELL_CASES["len-2"], "bad-index"), T.ManyProblem(CELL_CASES["len-64"], "bad-scalar"),
          T.ManyProblem(CELL_CASES["len-1"], "off-subgroup"), T.ManyProblem(CELL_CASES["four-interleaved"])]
    assert sorted({q.kind for q in qs}) == sorted(T.ManyProblem.STATUS)
    return qs, [q.args(mat) for q in qs]


def test_the_public_calls_agree(ctx, material):
    qs, problems = _kinds_pass(material)
    want = ([q.verdict for q in qs], [q.status for q in qs])
    assert want == ([True, True, False, False, False, False, True], [0, 0, 0, 3, 1, 2, 0])
    d = DeviceArrays(problems)
    lib = kzg.load_library()
    nb, lens, tabs, _keep = ctx._marshal_many(problems)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ver, st = (C.c_bool * nb)(), (C.c_int32 * nb)()
    res = lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex(ctx.handle, nb, vp(lens[0]), vp(tabs[0]), vp(lens[1]), vp(tabs[1]), vp(lens[2]), vp(tabs[2]),
                                                              vp(lens[3]), vp(tabs[3]), 0, ver, st)
    assert res.status == 0
    got = {"_many": ctx.verify_cell_kzg_proof_batch_many(problems), "_many_ex(0)": ([bool(v) for v in ver], list(st)),
           "_many_ex(leaf)": ctx.verify_cell_kzg_proof_batch_many(problems, leaf_transcript=True),
           "_many_device_ex(0)": d.call(ctx, False), "_many_device_ex(leaf)": d.call(ctx, True)}
    for call, g in got.items():
        assert g == want, (call, g)


def _invalid(res):
    lib = kzg.load_library()
    assert res.status == 1 and res.error_msg
    msg = C.string_at(res.error_msg).decode()
    lib.eth_kzg_free_error_message(res.error_msg)
    assert msg.startswith("InvalidInput"), msg


def test_call_level_errors_come_before_the_context_is_touched(ctx):
    lib = kzg.load_library()
    host = lambda n, flags: lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex(None, n, None, None, None, None, None, None, None, None, flags, None, None)  # noqa: E731
    dev = lambda n, cs, flags: lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex(None, n, cs, None, None, None, None, flags, None, None, None)  # noqa: E731
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)  # noqa: E731
    for flags in (2, 3, 1 << 31):
        _invalid(host(0, flags))
        _invalid(dev(0, None, flags))
    for flags in (0, LEAF):
        _invalid(host((1 << 24) + 1, flags))
        _invalid(dev((1 << 24) + 1, u64(0), flags))
        _invalid(dev(2, None, flags))            # NULL with problems
        _invalid(dev(2, u64(1, 4, 9), flags))    # the first entry is not 0
        _invalid(dev(3, u64(0, 4, 3, 9), flags))  # decreasing
        _invalid(dev(2, u64(0, 4, 3), flags))    # decreasing at the end
    # n_batches = 0 is Ok; a call of only empty problems verifies all of them (no array is read)
    for flags in (0, LEAF):
        for res in (lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex(ctx.handle, 0, None, None, None, None, None, None, None, None, flags, None, None),
                    lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex(ctx.handle, 0, None, None, None, None, None, flags, None, None, None)):
            assert res.status == 0
    empty = [([], [], [], [])] * 3
    for leaf in (False, True):
        assert ctx.verify_cell_kzg_proof_batch_many(empty, leaf_transcript=leaf) == ([True] * 3, [0] * 3)
        assert ctx.verify_cell_kzg_proof_batch_many_device([0, 0, 0, 0], 0, 0, 0, 0, leaf_transcript=leaf) == ([True] * 3, [0] * 3)
    assert lib.eth_kzg_amd_abi_version() == 6


# ---- 4. addresses and ordering ------------------------------------------------------------------------------------------------------------------
def test_shifted_addresses_and_inputs_produced_on_the_callers_stream(ctx, material):
    import torch
    qs, problems = _kinds_pass(material)
    want = ([q.verdict for q in qs], [q.status for q in qs])
    stream = torch.cuda.Stream()
    d = DeviceArrays(problems, shift=8, stream=stream)
    assert all(p % 16 == 8 for p in d.ptrs)
    assert d.call(ctx, True, stream=stream.cuda_stream) == want
    d2 = DeviceArrays(problems, shift=8, stream=stream)
    assert d2.call(ctx, False, stream=stream.cuda_stream) == want
    stream.synchronize()


GAP_COUNTS = [3, 0, 2, 65, 1]


@pytest.mark.parametrize("wrong", [False, True])
def test_a_refused_problem_beside_an_empty_one_between_two_copy_runs(ctx, material, wrong):
    """Flat device arrays whose third problem is refused at validation (an index of 128): its two entries lie between the two runs of
    device-to-device copies, the empty problem beside it holds none.  Everything equals the pointer-list form of the same problems."""
    import random
    rng = random.Random("many-leaf:gap")
    cases = [T.CellCase("gap-%d" % n, [(rng.choice((0, 1, 2)), rng.randrange(T.N_CELLS)) for _ in range(n)]) for n in GAP_COUNTS]
    proofs = cases[3].args(material)[3]
    swap = next((i, j) for i in range(65) for j in range(i + 1, 65) if proofs[i] != proofs[j])
    qs = [T.ManyProblem(cases[0]), T.ManyProblem(cases[1], "empty"), T.ManyProblem(cases[2], "bad-index"),
          T.ManyProblem(cases[3], "swapped", swap) if wrong else T.ManyProblem(cases[3]), T.ManyProblem(cases[4])]
    problems = [q.args(material) for q in qs]
    assert [len(p[1]) for p in problems] == GAP_COUNTS and problems[2][1] == [problems[2][1][0], 128]
    accepted, verdicts = [0, 1, 3, 4], [True, True, False, not wrong, True]
    d = DeviceArrays(problems)
    assert list(d.starts) == [0, 3, 3, 5, 70, 71]
    for flags in (0, LEAF):
        lists = ctx.verify_cell_kzg_proof_batch_many(problems, leaf_transcript=bool(flags))
        assert lists == (verdicts, [0, 0, 3, 0, 0]), (flags, lists)
        assert d.call(ctx, bool(flags)) == lists, flags
        rc, host = many_sums(ctx, problems, "host", flags)
        assert rc == 0
        rc, dev = many_sums(ctx, problems, "device", flags)
        assert rc == 0
        assert dev.status == [0, 0, 3, 0, 0] and host.status == dev.status, (flags, dev.status)
        assert dev.verified == host.verified == verdicts, (flags, dev.verified)
        # five problems under two host threads: the folded form; when the fold fails, the search's plan for four live problems
        plan = T.search_plan([True, False, False, True, True], verdicts, T.MANY_HOST_THREADS) if wrong else []
        form = (False, True, bool(plan), 0 if wrong else 1)
        assert (dev.small, dev.folded, dev.searched, dev.fold_verdict) == form == (host.small, host.folded, host.searched, host.fold_verdict), flags
        for b in accepted:
            assert dev.sums[b] == host.sums[b] and dev.rho[b] == host.rho[b] and dev.digests[b] == host.digests[b], (flags, b)
        assert dev.rho[1] == dev.rho[2] == 0 and all(dev.rho[b] for b in (0, 3, 4))
        assert dev.fold == host.fold and dev.fold != bytes(96), flags
        assert dev.n_probes == host.n_probes == len(plan) and dev.probes == host.probes, flags
        assert [(lo, hi, ok) for lo, hi, _, ok in dev.probes] == plan, flags
        if flags:
            assert dev.leaves == host.leaves and dev.leaves[3:5] == [bytes(32)] * 2 and bytes(32) not in dev.leaves[:3] + dev.leaves[5:]


# ---- 5. cuts ------------------------------------------------------------------------------------------------------------------------------------
def _tiled(mat, n_problems, wrong, tail_cells=0):
    """n_problems copies of one 128-cell problem (+ one of tail_cells), problem `wrong` with two proofs exchanged, as flat device arrays
    built by tiling on the device -> (cell_starts, pointers, keep-alive, the one problem, its swapped form)"""
    import torch
    one = CELL_CASES["all-128-indices"].args(mat)
    proofs = one[3]
    i, j = next((i, j) for i in range(128) for j in range(i + 1, 128) if proofs[i] != proofs[j])
    bad = (one[0], one[1], one[2], [proofs[j] if k == i else proofs[i] if k == j else proofs[k] for k in range(128)])
    base = DeviceArrays([one])
    total = 128 * n_problems + tail_cells
    keep, ptrs = [base], []
    for a, width in zip(base.keep, (48, 8, 2048, 48)):
        t = a.repeat(n_problems + (1 if tail_cells else 0))[:total * width].contiguous()
        keep.append(t)
        ptrs.append(t.data_ptr())
    keep[4][wrong * 128 * 48:(wrong + 1) * 128 * 48] = torch.frombuffer(bytearray(b"".join(bad[3])), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    starts = [128 * b for b in range(n_problems + 1)] + ([total] if tail_cells else [])
    return starts, ptrs, keep, one, bad


def test_a_call_cut_into_parts(ctx, material):
    """192 problems of 128 cells: three concurrent parts; one wrong problem in the second"""
    n, wrong = 192, 100
    starts, ptrs, _keep, one, bad = _tiled(material, n, wrong)
    want = ([b != wrong for b in range(n)], [0] * n)
    assert ctx.verify_cell_kzg_proof_batch_many([bad if b == wrong else one for b in range(n)], leaf_transcript=True) == want
    assert ctx.verify_cell_kzg_proof_batch_many_device(starts, *ptrs, leaf_transcript=True) == want


def test_a_call_of_1026_problems(ctx, material):
    """1025 problems of 128 cells and one of 3: 131203 cells, more than one pass may hold (131072).  A call of 192 problems or more is
    cut into three concurrent parts first, and each part of this one fits one pass: it checks the cut of cell_starts at problem
    boundaries on a call of this size, not a second chunk (test_a_second_chunk_on_one_slot does that)"""
    n, wrong = 1025, 1000
    starts, ptrs, _keep, _one, _bad = _tiled(material, n, wrong, tail_cells=3)
    assert len(starts) == n + 2 and starts[-1] == 131203
    t0 = time.perf_counter()
    got = ctx.verify_cell_kzg_proof_batch_many_device(starts, *ptrs, leaf_transcript=True)
    print("1026 problems, device flagged: %.3f s" % (time.perf_counter() - t0))
    assert got == ([b != wrong for b in range(n + 1)], [0] * (n + 1))


CHUNK_CELLS, SPLIT_MIN_PROBLEMS = 131072, 192  # engine.hpp: VM_CHUNK_CELLS, VM_SPLIT_MIN_PROBLEMS


def test_a_second_chunk_on_one_slot(ctx, material):
    """Fewer than 192 problems (no parts) with more than 131072 cells: the chunk loop runs twice on one slot.  136 problems of 1024
    cells (the 128-cell problem eight times over, tiled on the device); problem 127 is refused (an index of 128), so the first pass
    takes the problems 0 .. 128 -- 128 live ones, exactly 131072 cells, in two runs of device-to-device copies around the gap -- and
    the second pass the problems 129 .. 135, where 131 is refused too (a gap behind a chunk's begin) and 133, behind it, has two
    proofs exchanged: the pass's own indices, rows and positions, the caller's absolute entries and the pass-relative place in the
    arena all differ there from the first pass's"""
    import torch
    n, reps, refused, wrong = 136, 8, (127, 131), 133
    per = 128 * reps
    assert n < SPLIT_MIN_PROBLEMS and n * per > CHUNK_CELLS
    live_cells = [0 if b in refused else per for b in range(n)]
    first = next(b for b in range(n + 1) if sum(live_cells[:b + 1]) > CHUNK_CELLS)  # the first problem of the second pass
    assert first == 129 and sum(live_cells[:first]) == CHUNK_CELLS and refused[0] == first - 2 and first < refused[1] < wrong
    assert sum(live_cells[first:]) <= CHUNK_CELLS and sum(1 for c in live_cells[first:] if c) > 2 * T.MANY_HOST_THREADS  # two passes; no short chain
    one = CELL_CASES["all-128-indices"].args(material)
    proofs = one[3]
    i, j = next((i, j) for i in range(128) for j in range(i + 1, 128) if proofs[i] != proofs[j])
    swapped = [proofs[j] if k == i else proofs[i] if k == j else proofs[k] for k in range(128)]
    base = DeviceArrays([one])
    comm, idx, cells, prf = [a.repeat(n * reps).contiguous() for a in base.keep]
    assert [t.numel() for t in (comm, idx, cells, prf)] == [n * per * w for w in (48, 8, 2048, 48)]
    prf[wrong * per * 48:(wrong * per + 128) * 48] = torch.frombuffer(bytearray(b"".join(swapped)), dtype=torch.uint8).cuda()
    for b in refused:  # the last index of the problem: 128, little-endian
        idx[((b + 1) * per - 1) * 8:(b + 1) * per * 8] = torch.tensor([128, 0, 0, 0, 0, 0, 0, 0], dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    starts = [per * b for b in range(n + 1)]
    t0 = time.perf_counter()
    got = ctx.verify_cell_kzg_proof_batch_many_device(starts, comm.data_ptr(), idx.data_ptr(), cells.data_ptr(), prf.data_ptr(), leaf_transcript=True)
    print("136 problems of 1024 cells, device flagged, two chunks: %.3f s" % (time.perf_counter() - t0))
    assert got == ([b not in refused and b != wrong for b in range(n)], [3 if b in refused else 0 for b in range(n)])


def test_a_problem_beyond_the_size_bound_is_refused_unread(ctx, material):
    """cell_starts may state a problem of 2^24 cells: it is refused with status 3 before anything of it is read or sized (the arrays
    here end where it begins), and the problems around it keep their verdicts"""
    qs, problems = _kinds_pass(material)
    want = ([q.verdict for q in qs] + [False, True], [q.status for q in qs] + [3, 0])
    d = DeviceArrays(problems)
    starts = list(d.starts) + [d.starts[-1] + (1 << 24)] * 2  # + a problem of 2^24 cells and an empty one behind it
    for leaf in (True, False):
        assert ctx.verify_cell_kzg_proof_batch_many_device(starts, *d.ptrs, leaf_transcript=leaf) == want, leaf
    only = [0, 1 << 24]
    assert ctx.verify_cell_kzg_proof_batch_many_device(only, *d.ptrs, leaf_transcript=True) == ([False], [3])


# ---- 6. the reference's vectors -----------------------------------------------------------------------------------------------------------------
GOLDEN = sorted(vectors.load("verify_cell_kzg_proof_batch").items())


def _flattenable(i):
    return len(i["commitments"]) == len(i["cell_indices"]) == len(i["cells"]) == len(i["proofs"]) and all(len(c) == 48 for c in i["commitments"]) \
        and all(len(p) == 48 for p in i["proofs"]) and all(len(c) == 2048 for c in i["cells"])


def test_the_reference_vectors_as_the_problems_of_one_call(ctx):
    assert len(GOLDEN) == 30
    problems = [(c["input"]["commitments"], c["input"]["cell_indices"], c["input"]["cells"], c["input"]["proofs"]) for _, c in GOLDEN]
    outputs = [c["output"] for _, c in GOLDEN]
    unflagged = ctx.verify_cell_kzg_proof_batch_many(problems)
    assert [v if s == 0 else None for v, s in zip(*unflagged)] == outputs  # Err cases: a status other than 0
    assert ctx.verify_cell_kzg_proof_batch_many(problems, leaf_transcript=True) == unflagged
    # the flat form has one length per problem and fixed widths: a problem the reference refuses for its lengths goes in as one cell with
    # the index 128, which the flat form refuses with the same status 3
    refused = ([bytes(48)], [128], [bytes(2048)], [bytes(48)])
    flat = [p if _flattenable(c["input"]) else refused for p, (_, c) in zip(problems, GOLDEN)]
    assert all(unflagged[1][b] == 3 for b in range(30) if flat[b] is refused) and sum(p is not refused for p in flat) >= 20
    assert DeviceArrays(flat).call(ctx, True) == unflagged


# ---- 7. a device list ---------------------------------------------------------------------------------------------------------------------------
def test_device_list_host_form_sliced_device_form_by_owner(ctx, material):
    qs, problems = _kinds_pass(material)
    want = ([q.verdict for q in qs], [q.status for q in qs])
    multi = _ctx(devices=[0, 0], ETH_KZG_AMD_HOST_THREADS=str(T.MANY_HOST_THREADS))
    try:
        assert multi.verify_cell_kzg_proof_batch_many(problems, leaf_transcript=True) == want == ctx.verify_cell_kzg_proof_batch_many(problems, leaf_transcript=True)
        d = DeviceArrays(problems)
        assert d.call(multi, True) == want == d.call(ctx, True)
        assert d.call(multi, False) == want
        # all four pointers are resolved: a host address in any place is InvalidInput (it is never dereferenced on the device)
        host = np.zeros(d.starts[-1] * 2048, dtype=np.uint8)
        for c in (multi, ctx):
            for k in range(4):
                ptrs = list(d.ptrs)
                ptrs[k] = host.ctypes.data
                for leaf in (True, False):
                    with pytest.raises(kzg.KzgError, match="InvalidInput"):
                        c.verify_cell_kzg_proof_batch_many_device(d.starts, *ptrs, leaf_transcript=leaf)
        assert d.call(multi, True) == want  # and the context goes on working
    finally:
        multi.close()


# ---- 8. four threads ----------------------------------------------------------------------------------------------------------------------------
def test_four_threads_each_get_their_own_verdicts(ctx, material):
    qs, problems = _kinds_pass(material)
    base = ([q.verdict for q in qs], [q.status for q in qs])
    calls = [(problems[t:] + problems[:t], (base[0][t:] + base[0][:t], base[1][t:] + base[1][:t])) for t in range(4)]
    assert len({tuple(w[1]) for _, w in calls}) == 4
    got, errors = [None] * 4, []

    def run(t):
        try:
            for _ in range(3):
                got[t] = ctx.verify_cell_kzg_proof_batch_many(calls[t][0], leaf_transcript=True)
                assert got[t] == calls[t][1], t
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    th = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    assert [g for g in got] == [w for _, w in calls]
