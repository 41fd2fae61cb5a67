"""The prover's G1 stage alone -- from the 128 sums a blob's fixed-base MSMs leave to its 128 proofs' bytes -- through
eth_kzg_amd_test_proofs_from_sums, which makes the launches compute_cells_and_kzg_proofs makes behind the MSM (k_g1slp.hip over one
of six compiled programs, or k_g1circ.hip for one or two blobs, then k_g1_compress), on sums real blobs never give: lanes planned by
tests/linmap_model.py so that every kind of addition of every program meets an identity, a = b and a = -b while the other lanes of
its wave run the regular formulas (tests/test_linmap_stage_host.py computes that coverage on the CPU).  Expected bytes come from the
map's definition in exact integers and the oracle's scalar multiplication; every comparison is byte for byte.

Run on the MI355X box:  python -m pytest tests/test_gpu_g1_stage.py -m gpu -q
"""
import ctypes as C
import importlib
import os
import random

import numpy as np
import pytest

import device_ops as D
import g1_stage_cases as S
import linmap_model as M
import synth

pytestmark = pytest.mark.gpu
kzg = importlib.import_module("rust-eth-kzg_amd")
R = M.R


@pytest.fixture(scope="module")
def ctx():
    """one context on small tables (the hook does not touch them; the product-stage test runs two small MSMs on them)"""
    import torch
    torch.cuda.init()  # torch initialises its HIP state before the engine creates its streams
    saved = os.environ.get("ETH_KZG_AMD_TABLE_GB")
    os.environ["ETH_KZG_AMD_TABLE_GB"] = "8"
    try:
        c = kzg.DASContext(use_precomp=True)
    finally:
        if saved is None:
            os.environ.pop("ETH_KZG_AMD_TABLE_GB", None)
        else:
            os.environ["ETH_KZG_AMD_TABLE_GB"] = saved
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib():
    return kzg.load_library()


# ---- the programs the context runs are the programs the CPU plan was made for ------------------------------------------------------
@pytest.mark.parametrize("program", range(6))
def test_g1_stage_program_uploaded_is_the_one_dumped_on_the_host(ctx, lib, program):
    words = np.zeros(1 << 16, dtype=np.uint32)
    launches = np.zeros((64, 3), dtype=np.int32)
    consts = np.zeros((1024, 32), dtype=np.uint8)
    nw, nl, nc, slots = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
    rc = lib.eth_kzg_amd_test_linmap_program(ctx.handle, program, words.ctypes.data, words.size, C.byref(nw), launches.ctypes.data, 64,
                                             C.byref(nl), C.byref(slots), consts.ctypes.data, 1024, C.byref(nc))
    assert rc == 0
    p = M.programs()[program]
    assert slots.value == p.n_slots
    assert [tuple(int(v) for v in l) for l in launches[:nl.value]] == p.launches
    assert words[:nw.value].tolist() == [v for op in p.ops for v in op]
    assert [int.from_bytes(consts[i].tobytes(), "big") for i in range(nc.value)] == p.consts
    tiny = np.zeros(4, dtype=np.uint32)  # a buffer that is too small is refused, with the counts
    assert lib.eth_kzg_amd_test_linmap_program(ctx.handle, program, tiny.ctypes.data, 4, C.byref(nw), launches.ctypes.data, 64, C.byref(nl),
                                               C.byref(slots), consts.ctypes.data, 1024, C.byref(nc)) == 3
    assert nw.value == 4 * len(p.ops)


# ---- the hook is the product's stage ---------------------------------------------------------------------------------------------
def _prover_scalars(lib, ctx, blobs):
    n = len(blobs)
    max_words = 4 * n * 8192 * 8
    scalars = np.zeros(max_words, dtype=np.uint32)
    cells = np.zeros((n, 128 * 2048), dtype=np.uint8)
    proofs = np.zeros((n, 128 * 48), dtype=np.uint8)
    status = np.zeros(n, dtype=np.int32)
    n_words, fused = C.c_uint64(0), C.c_int32(-1)
    rc = lib.eth_kzg_amd_test_prover_scalars(ctx.handle, n, b"".join(blobs), scalars.ctypes.data, max_words, C.byref(n_words),
                                             cells.ctypes.data, proofs.ctypes.data, status.ctypes.data, C.byref(fused))
    assert rc == 0 and status.tolist() == [0] * n
    segs = n_words.value // (n * 8192 * 8)
    assert segs * n * 8192 * 8 == n_words.value
    return scalars[:n_words.value].reshape(segs * n, 128 * 64, 8), proofs, segs


def _recombined_be(halves):
    """[m][8192][8] words (k1 | k2, sign in bit 127 of each half) -> the scalars k1 + k2 lambda mod r, canonical big-endian"""
    lam = M.programs()[0].lam
    out = bytearray()
    for row in halves.reshape(-1, 8):
        v = [int(x) for x in row]
        k = []
        for h in (v[:4], v[4:]):
            mag = sum(x << (32 * i) for i, x in enumerate(h))
            neg, mag = mag >> 127, mag & ((1 << 127) - 1)
            k.append(-mag if neg else mag)
        out += ((k[0] + k[1] * lam) % R).to_bytes(32, "big")
    return bytes(out)


@pytest.mark.parametrize("n", [3, 1])
def test_g1_stage_hook_gives_the_provers_proofs_from_the_provers_sums(ctx, lib, n):
    """The prover's own scalars (eth_kzg_amd_test_prover_scalars), its MSM on them (eth_kzg_amd_test_fixed_msm, per segment copy
    for the single blob), the sums re-encoded with fresh Z: the hook turns them into the proof bytes the prover returned."""
    blobs = [synth.seeded_blob(s) for s in range(n)]
    halves, proofs, segs = _prover_scalars(lib, ctx, blobs)
    assert segs == (4 if n == 1 else 1)
    m = segs * n
    sums = np.zeros((m, 128, 48), dtype=np.uint8)
    assert lib.eth_kzg_amd_test_fixed_msm(ctx.handle, _recombined_be(halves), m, sums.ctypes.data) == 0
    rng = random.Random(90 + n)
    words = np.zeros((128, m, 39), dtype=np.int64)
    for lane in range(m):
        for j in range(128):
            words[j, lane] = D.enc_jacs(S.decompress(sums[lane, j].tobytes()), rng, extreme=rng.random() < 0.25)
    words = np.ascontiguousarray((words & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
    rc, got = S.proofs_from_sums(lib, ctx.handle, -1, n, words)
    assert rc == 0
    for b in range(n):
        assert got[b] == proofs[b].tobytes(), (n, b)


def test_g1_stage_hook_refuses_what_it_cannot_run(ctx, lib):
    words = np.zeros((128, 2, 39), dtype=np.int32)
    out = np.zeros(2 * 128 * 48, dtype=np.uint8)
    call = lambda program, n: lib.eth_kzg_amd_test_proofs_from_sums(ctx.handle, program, n, words.ctypes.data, out.ctypes.data)  # noqa: E731
    assert call(2, 1) == 3 and call(0, 2) == 3  # a forced program where the circulant form runs
    assert call(-2, 12) == 3 and call(6, 12) == 3 and call(-1, 0) == 3 and call(-1, 257) == 3


# ---- the compiled linear map: six programs x three batch shapes ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [12, 40, 70])
@pytest.mark.parametrize("program", range(6))
def test_g1_stage_linear_map_on_planned_degenerate_lanes(ctx, lib, program, n):
    """n = 12: four lanes per blob in the multiplications, and in the additions of a launch of at most 256 operations (a lane per
    blob in the larger launches).  n = 40: two lanes per blob in the multiplications of program 3 (the engine's pick there), a lane
    per blob in the others; additions as for 12.  n = 70: a lane per blob, two lane groups, six lanes of the second in use.  The
    program's degenerate lanes sit at lane 0, n - 1 (which the padding lanes repeat), a middle lane, 15, 63 and 64; generic and
    all-identity lanes lie between them."""
    for k, (batch, vectors) in enumerate(S.linmap_batches(program, n)):
        S.check_linmap_batch(lib, ctx.handle, program, program, n, batch, vectors, seed=1000 * program + 10 * n + k)


@pytest.mark.parametrize("n,program", [(3, 2), (64, 3)])
def test_g1_stage_linear_map_as_the_engine_picks_it(ctx, lib, n, program):
    """program -1: what the prover runs at this batch size (engine.hip: pick_slp_program -- Karatsuba with four lanes per blob for 3
    blobs; engine_prover.hip: the 456-multiplication program with two lanes per blob for a full lane group), on the lanes planned for
    that program, and the same lanes with that program forced"""
    if n == 3:
        _, lanes, generic = S.plan(program)
        batches = [(b, [lanes[0], generic[0], lanes[1]]) for b in [[("d", 0), ("g", 0), ("d", 1)]]]
    else:
        batches = S.linmap_batches(program, n)
    for k, (batch, vectors) in enumerate(batches):
        S.check_linmap_batch(lib, ctx.handle, program, -1, n, batch, vectors, seed=7000 + 10 * n + k)
        S.check_linmap_batch(lib, ctx.handle, program, program, n, batch, vectors, seed=7000 + 10 * n + k)


# ---- the circulant form: one and two blobs ------------------------------------------------------------------------------------------
def _circulant_vectors():
    rng = random.Random(4141)
    pool = M.pool_scalars()
    pick = lambda: pool[rng.randrange(len(pool))]  # noqa: E731
    generic = [pick() for _ in range(128)]
    one_identity = [pick() for _ in range(128)]
    one_identity[37] = 0
    c = pick()
    alternating = [c if j % 2 == 0 else R - c for j in range(128)]
    single = [0] * 128
    single[91] = pick()
    return {"generic": generic, "one identity": one_identity, "all identity": [0] * 128, "all equal": [c] * 128,
            "u[j+1] = -u[j]": alternating, "one non-zero": single, "generic 2": [pick() for _ in range(128)]}


@pytest.mark.parametrize("n", [1, 2])
def test_g1_stage_circulant_form(ctx, lib, n):
    """k_g1_dbl_table / k_g1_circ_sum (two blobs) and their four-lanes-per-chain forms with k_g1_circ_join (one blob) on generic
    inputs, one identity among them, all identities, 128 equal points, alternating signs and a single non-zero input, each with
    consistent segment copies 2^(32 s) u_j; the reference is the definition h_m = sum_j u_j omega^(-j m), out_k = sum_m h_m omega^(k m)."""
    _, _, segs = _prover_scalars(lib, ctx, [synth.seeded_blob(0)] * n)
    assert segs in (1, 2, 4)
    vec = _circulant_vectors()
    names = list(vec)
    groups = [[nm] for nm in names] if n == 1 else [names[i:i + 2] for i in range(0, len(names) - 1, 2)] + [["all identity", "generic 2"]]
    rng = random.Random(515 + n)
    for group in groups:
        rows = [[vec[group[lane % n]][j] * pow(2, (128 // segs) * (lane // n), R) % R for lane in range(segs * n)] for j in range(128)]
        rc, got = S.proofs_from_sums(lib, ctx.handle, -1, n, S.encode(rows, rng))
        assert rc == 0
        for b, nm in enumerate(group):
            want = S.expected_proofs(vec[nm], circulant=True)
            assert got[b] == want, (n, nm, S.wrong_lanes([got[b]], [want]))
