"""The fixed-base MSM kernels alone (csrc/k_msm_glv.inc: k_msm_glv_chunked, k_msm_glv_windowed<1|2>, k_msm_glv_flat<128|256>) through
eth_kzg_amd_test_fixed_msm_ex, one stated schedule at a time, on a setup whose 64 bases per group are ONE point: a gathered addition
then meets an accumulator equal or opposite to the next entry, equal and opposite fold operands, a k1 sum equal to +-lambda times the
k2 sum -- the exact slow paths of add_mixed, of the LDS folds and of the coop4 trees, inside the kernels.  tests/fixed_msm_cases.py
plans the scalars, models which addition is degenerate where (tests/test_fixed_msm_cases.py asserts that table without a GPU) and
states the reference: (sum of the scalars mod r) c_j G, byte for byte.  One context per table width, created and closed in turn."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import fixed_msm_cases as F
import oracle_lib
import setup_material as sm
import synth

pytestmark = pytest.mark.gpu
kzg = importlib.import_module("rust-eth-kzg_amd")
R = F.R
COLLIDING = [("colliding", 16), ("colliding", 15), ("colliding", 8)]
MAINNET = [("mainnet", 16), ("mainnet", 8)]
_ID = lambda p: "%s-w%d" % p  # noqa: E731
# (mode, slices): the smallest counts that change the code run -- flat: 256 threads up to 512 MSMs (4 slices of 128), 128 beyond; the
# windowed kernels: more than one block per group and a last block that is not full; four chunks: 55 idle lanes that fold
# identities, and a second block of slices
FORCED = [(0, 1), (0, 4), (0, 5), (0, 8), (3, 9), (3, 14), (1, 9), (1, 17), (2, 9), (2, 65)]


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    # the torch wheel carries its own HIP runtime: it must have been initialised before the engine's (tests/test_gpu_custom_setup.py)
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def msm_ctx(request):
    """(setup, width, context): width 16 = the suite's `max` budget, 15 = ETH_KZG_AMD_TABLE_GB unset, 8 = use_precomp=False.  Module
    scope and one parameter at a time: two wide tables do not fit one GPU."""
    setup, width = request.param
    saved = os.environ.get("ETH_KZG_AMD_TABLE_GB")
    if width == 16:
        os.environ["ETH_KZG_AMD_TABLE_GB"] = "max"
    else:
        os.environ.pop("ETH_KZG_AMD_TABLE_GB", None)
    c = None
    try:
        if setup == "colliding":
            c = kzg.DASContext.from_trusted_setup(*F.colliding_setup(), use_precomp=width != 8)
        else:
            c = kzg.DASContext(use_precomp=width != 8)
        assert c.window_bits() == width and c.tables_ready() == 1
        yield setup, width, c
    finally:
        if c is not None:
            c.close()
        if saved is None:
            os.environ.pop("ETH_KZG_AMD_TABLE_GB", None)
        else:
            os.environ["ETH_KZG_AMD_TABLE_GB"] = saved


def run(ctx, kind, mode, form, slices):
    """slices: one bytes object per slice ([groups][64][32]) -> (out[slice][group] -> 48 bytes, modes launched)"""
    lib = kzg.load_library()
    n, groups = len(slices), F.groups_of(kind)
    buf = b"".join(slices)
    assert len(buf) == n * groups * 64 * 32
    out = C.create_string_buffer(n * groups * 48)
    modes = (C.c_int32 * 5)()
    assert lib.eth_kzg_amd_test_fixed_msm_ex(ctx.handle, kind, mode, form, buf, n, out, modes) == 0, (kind, mode, form, n)
    raw = out.raw
    return (lambda s, j: raw[(s * groups + j) * 48:(s * groups + j + 1) * 48]), list(modes[1:1 + modes[0]])


def table_width(ctx, kind):
    out8 = (C.c_int64 * 8)()
    assert kzg.load_library().eth_kzg_amd_test_table_info(ctx.handle, kind, 0, out8, None, 0) == 0
    assert out8[3] == 1 and out8[1] == F.groups_of(kind) and out8[2] == 64
    return int(out8[0])


_POOLS, _SLICES = {}, {}


def pool(kind):
    if kind not in _POOLS:
        _POOLS[kind] = F.RandomSlices(F.groups_of(kind), 77 + kind)
    return _POOLS[kind]


def case_slice(width, case, form, kind):
    key = (width, case.name, form, kind)
    if key not in _SLICES:
        _SLICES[key] = F.slice_bytes(case, form, F.groups_of(kind))
    return _SLICES[key]


def check_planned(ctx, kind, width, mode, n, case_list, want_modes=None):
    """Every case in both scalar forms at n slices: the planned slices at the even places (each case in all groups of its slice), seeded
    random slices between them so that the lanes of a wave take different paths; every output compared."""
    groups, rnd = F.groups_of(kind), pool(kind)
    places = list(range(0, n, 2))
    wrong = []
    for form in (0, 1):
        todo = [c for c in case_list if form == 1 or not c.minus_zero]
        for first in range(0, len(todo), len(places)):
            batch = (todo[first:first + len(places)] * len(places))[:len(places)]  # a short last batch repeats its cases
            slices = [case_slice(width, batch[s // 2], form, kind) if s % 2 == 0 else rnd.bytes[form][(s // 2) % 3] for s in range(n)]
            got, modes = run(ctx, kind, mode, form, slices)
            assert modes == (want_modes or [mode]), (modes, mode, n)
            for s in range(n):
                for j in range(groups):
                    total = batch[s // 2].total() if s % 2 == 0 else rnd.total((s // 2) % 3, j)
                    if got(s, j) != F.expected(kind, j, total):
                        wrong.append((form, batch[s // 2].name if s % 2 == 0 else "random %d" % ((s // 2) % 3), s, j))
    assert not wrong, (len(wrong), wrong[:12])


@pytest.mark.parametrize("mode,n", FORCED)
@pytest.mark.parametrize("msm_ctx", COLLIDING, indirect=True, ids=_ID)
def test_forced_schedules_on_colliding_bases(msm_ctx, mode, n):
    _, width, ctx = msm_ctx
    check_planned(ctx, 0, width, mode, n, F.cases(width))


def engine_modes(n, width, cus, groups=128):
    """launch_msm_range's rule: up to 8 slices a block per MSM; two lanes per window while that fills at most half of the chip's wave
    slots (8 per CU); four chunks once they fill all of them; else a lane per window -- and when those lanes exceed one round of the
    slots by at most a quarter, the slices of the first round that way and the rest on their own (a block per MSM up to 8, else two lanes)."""
    W, slots, msms = -(-128 // width), cus * 8, groups * n
    if n <= 8:
        return [0]
    if (msms * 4 * W + 63) // 64 <= slots // 2:
        return [3]
    if (msms * 4 + 63) // 64 >= slots:
        return [2]
    lanes, n_a = msms * 2 * W, slots * 64 // (groups * 2 * W)
    return [1, 0 if n - n_a <= 8 else 3] if slots * 64 < lanes <= slots * 80 and 1 <= n_a < n else [1]


@pytest.mark.parametrize("msm_ctx", COLLIDING, indirect=True, ids=_ID)
def test_the_engines_own_choice_reports_its_kernels(msm_ctx):
    """Mode -1 at the counts where the choice changes, and at the overflow form.  On the 256 CUs of an MI355X: eight windows 1, 8 -> flat;
    9, 16 -> two lanes; 17 -> a lane; 65 -> 64 slices a lane per window + 1 flat.  Nine windows: 9 -> two lanes, 16 and 17 -> a lane
    (two lanes stop at 14), 57 -> 56 + 1.  Sixteen windows: two lanes stop at 8, where flat still rules, so 9, 16, 17 -> a lane; a round
    is 32 slices: 33 -> 32 + 1 (neither 57 nor 65 overflows there: beyond a quarter round it is one launch)."""
    import torch
    _, width, ctx = msm_ctx
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    overflow = {16: 65, 15: 57, 8: 33}[width]
    cs = F.cases(width)
    seen = []
    for k, n in enumerate((1, 8, 9, 16, 17, overflow)):
        want = engine_modes(n, width, cus)
        seen.append(want)
        check_planned(ctx, 0, width, -1, n, cs[5 * k:5 * k + 5], want_modes=want)
    if cus == 256:
        assert seen == {16: [[0], [0], [3], [3], [1], [1, 0]], 15: [[0], [0], [3], [1], [1], [1, 0]], 8: [[0], [0], [1], [1], [1], [1, 0]]}[width]


@pytest.mark.parametrize("msm_ctx", COLLIDING, indirect=True, ids=_ID)
def test_commitment_table_group_sums_on_colliding_bases(msm_ctx):
    """Kind 1: the 64 group sums of a slice before the commitment's fold; every base is G.  The commitment table's width is the
    context's own (nine windows beside an FK20 table of width 16 or 15, sixteen windows without precomputation)."""
    _, width, ctx = msm_ctx
    cw = table_width(ctx, 1)
    assert cw == (8 if width == 8 else 15)
    cs = F.cases(cw)
    for mode, n in ((0, 4), (0, 9), (3, 9), (1, 17), (2, 9)):
        check_planned(ctx, 1, cw, mode, n, cs)


def _coeff_blobs():
    rng = np.random.default_rng(3)
    seeded = F.blob_coefficients(synth.seeded_blob(951))
    mirrored = list(seeded)
    for i in range(64):
        mirrored[64 * 9 + i] = (R - mirrored[64 * 5 + i]) % R
    firsts = [int(rng.integers(1, 1 << 62))] * 64
    return {
        "all ones": [1] * 4096,                      # every FK20 scalar and every commitment group sum is the same
        "alternating": [1, R - 1] * 2048,            # every commitment group sum is the identity
        "group 9 = -group 5": mirrored,
        "seeded": seeded,
        "degree below 64, equal": firsts,            # the quotient is zero: every proof is the identity
        "degree below 64, alternating": [v if i % 2 == 0 else R - v for i, v in enumerate(firsts)],
        "blocks equal": ([7] * 64 + [R - 7] * 64) * 32,
    }


@pytest.fixture(scope="module")
def colliding_oracle():
    """The CPU oracle computes on this setup too (its adders take equal and opposite points): a second reference beside the closed forms."""
    o = sm.SetupOracle(*F.colliding_setup())
    yield o
    o.close()


@pytest.fixture(scope="module")
def coeff_blobs():
    co = _coeff_blobs()
    return {k: (v + [0] * (4096 - len(v)), F.blob_of_coefficients(v)) for k, v in co.items()}


@pytest.mark.parametrize("msm_ctx", COLLIDING, indirect=True, ids=_ID)
def test_commitments_equal_their_closed_form(msm_ctx, coeff_blobs, colliding_oracle):
    """tau = 1: the commitment is p(1) G, and p(1) is the blob's element 0."""
    _, _, ctx = msm_ctx
    names = sorted(coeff_blobs)
    want = {}
    for k in names:
        coeffs, blob = coeff_blobs[k]
        assert F.commitment_scalar(coeffs, 1) == int.from_bytes(blob[:32], "big")
        want[k] = F.times_g(F.commitment_scalar(coeffs, 1))
        assert ctx.blob_to_kzg_commitment(blob) == want[k] == colliding_oracle.blob_to_kzg_commitment(blob), k
    assert want["alternating"] == F.IDENTITY
    for n in (3, 9, 70):
        batch = [names[i % len(names)] for i in range(n)]
        st, comms = ctx.blob_to_kzg_commitment_batch([coeff_blobs[k][1] for k in batch])
        assert list(st) == [0] * n
        assert [k for k, cm in zip(batch, comms) if cm != want[k]] == [], n


_PROOFS = {}


def _want_proofs(name, coeffs):
    if name not in _PROOFS:
        _PROOFS[name] = [F.times_g(F.proof_scalar(coeffs, k, 1)) for k in range(128)]
    return _PROOFS[name]


@pytest.mark.parametrize("n", [1, 3, 9, 70])
@pytest.mark.parametrize("msm_ctx", COLLIDING, indirect=True, ids=_ID)
def test_proofs_equal_their_closed_form(msm_ctx, coeff_blobs, oracle, colliding_oracle, n):
    """proof_k = q_k(1) G with q_k = (p - I_k) / (X^64 - h_k^64) by polynomial division (cell 0 has h^64 = 1 = tau^64); the cells do
    not depend on the setup and are the mainnet oracle's."""
    _, _, ctx = msm_ctx
    names = ["all ones", "blocks equal", "degree below 64, equal", "degree below 64, alternating", "seeded"]
    batch = [names[i % len(names)] for i in range(n)]
    status, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch([coeff_blobs[k][1] for k in batch])
    assert list(status) == [0] * n
    for i, k in enumerate(batch):
        want = _want_proofs(k, coeff_blobs[k][0])
        assert [c for c in range(128) if proofs[i][c] != want[c]] == [], (n, i, k)
    assert _want_proofs("degree below 64, equal", coeff_blobs["degree below 64, equal"][0]) == [F.IDENTITY] * 128
    assert list(proofs[n - 1]) == list(colliding_oracle.compute_cells_and_kzg_proofs(coeff_blobs[batch[n - 1]][1])[1])
    for i in sorted({0, n - 1}):
        assert list(cells[i]) == list(oracle.compute_cells_and_kzg_proofs(coeff_blobs[batch[i]][1])[0]), (n, i)


_MAINNET_WANT = {}


@pytest.mark.parametrize("msm_ctx", MAINNET, indirect=True, ids=_ID)
def test_forced_schedules_on_the_mainnet_bases_at_the_recodings_edges(msm_ctx):
    """The Booth-edge scalars of tests/test_gpu_tables.py (_stage_scalars) through every forced schedule against oracle_lib.g1_msm: the
    decoders of the flat and the two-lane kernels (booth_mem) at stage level.  And the commitment table's groups on the mainnet points."""
    import test_gpu_fullsize as full
    import test_gpu_tables as tables
    _, width, ctx = msm_ctx
    sc = tables._stage_scalars(width)
    slices = [b"".join(s) for s in sc]
    compared = [(0, 0), (0, 1), (0, 2), (2, 64), (8, 77)] + [(2 + j % 7, j) for j in range(128)]
    for m, j in compared:
        if (width, m, j) not in _MAINNET_WANT:
            pts = b"".join(full._fk20_base_column(i)[j] for i in range(64))
            _MAINNET_WANT[(width, m, j)] = oracle_lib.g1_msm(pts, b"".join(sc[m][j * 64:(j + 1) * 64]))
    for mode, n in ((0, 4), (0, 9), (1, 9), (3, 9), (2, 9)):
        got, modes = run(ctx, 0, mode, 0, slices[:n])
        assert modes == [mode]
        assert all(got(1, j) == F.IDENTITY for j in range(128)), (mode, n)
        wrong = [(m, j) for m, j in compared if m < n and got(m, j) != _MAINNET_WANT[(width, m, j)]]
        assert not wrong, (width, mode, n, wrong[:10])
    g1 = F.sm.mainnet_points()[0]
    rnd = pool(1)
    for mode, n in ((0, 3), (3, 9), (1, 9), (2, 9)):
        got, _ = run(ctx, 1, mode, 1, [rnd.bytes[1][s % 3] for s in range(n)])
        for s, j in ((0, 0), (1, 63), (n - 1, 17)):
            scal = b"".join(F.join(k1, k2).to_bytes(32, "big") for k1, k2 in rnd.halves[s % 3][j])
            assert got(s, j) == oracle_lib.g1_msm(g1[48 * 64 * j:48 * 64 * (j + 1)], scal), (mode, n, s, j)
