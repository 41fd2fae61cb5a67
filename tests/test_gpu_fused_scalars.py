"""k_coeffs_to_cells_scalars (the cells' transform that also emits the FK20 scalars, and copies cells 0-63 of an accepted blob from its
bytes) against the pair of kernels it replaces, k_coeffs_to_cells + k_fk20_scalars: the MSM's scalars word for word through
eth_kzg_amd_test_prover_scalars, cells and proofs byte for byte against the pair and against the CPU oracle.  Two contexts on the start
tables, one per value of ETH_KZG_AMD_FUSED_SCALARS, so that both kernels run at every batch size -- one block, two blocks (with the
segment copies of the smallest batches), one blob past a lane group -- and a third with the knob unset for the engine's own choice.

Run on the MI355X box:  python -m pytest tests/test_gpu_fused_scalars.py -m gpu -q
"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
kzg = importlib.import_module("rust-eth-kzg_amd")

R_MINUS_1 = (synth.R - 1).to_bytes(32, "big")


def _blob(kind, seed=0):
    if kind == "random":
        a = np.random.RandomState(4200 + seed).randint(0, 256, size=(4096, 32), dtype=np.uint8)
        a[:, 0] &= 0x3F  # < 2^254 < r
        return a.tobytes()
    if kind == "zero":
        return bytes(131072)
    if kind == "r-1":
        return R_MINUS_1 * 4096
    at = {"e0": 0, "e63": 63, "e64": 64, "e4095": 4095}[kind]  # one non-zero element
    value = (0x1234567 + at).to_bytes(32, "big")
    return bytes(32 * at) + value + bytes(32 * (4095 - at))


SPECIAL = ["zero", "r-1", "e0", "e4095", "e63", "e64"]


def _context(fused):
    """a context on the start tables (2.4 GB, no wide build) under ETH_KZG_AMD_FUSED_SCALARS = fused (None: unset)"""
    import torch
    torch.cuda.init()  # torch initialises its HIP state before the engine creates its streams
    saved = os.environ.pop("ETH_KZG_AMD_FUSED_SCALARS", None)
    if fused is not None:
        os.environ["ETH_KZG_AMD_FUSED_SCALARS"] = str(fused)
    try:
        return kzg.DASContext(use_precomp=False)  # the knobs are read once, here
    finally:
        os.environ.pop("ETH_KZG_AMD_FUSED_SCALARS", None)
        if saved is not None:
            os.environ["ETH_KZG_AMD_FUSED_SCALARS"] = saved


@pytest.fixture(scope="module")
def contexts():
    made = {}
    try:
        for name, fused in (("pair", 0), ("fused", 1), ("auto", None)):
            made[name] = _context(fused)
        yield made
    finally:
        for c in made.values():
            c.close()


_ORACLE = {}


def _expected(oracle, blob):
    """the oracle's (cells, proofs) of one blob as two byte strings, computed once per distinct blob of the module"""
    if blob not in _ORACLE:
        ec, ep = oracle.compute_cells_and_kzg_proofs(blob)
        _ORACLE[blob] = (b"".join(ec), b"".join(ep))
    return _ORACLE[blob]


def _run(ctx, blobs):
    """-> (scalar words, cells [n][262144], proofs [n][6144], status, launches of the fused kernel)"""
    lib = kzg.load_library()
    n = len(blobs)
    max_words = 4 * n * 8192 * 8
    scalars = np.zeros(max_words, dtype=np.uint32)
    cells = np.zeros((n, 128 * 2048), dtype=np.uint8)
    proofs = np.zeros((n, 128 * 48), dtype=np.uint8)
    status = np.zeros(n, dtype=np.int32)
    n_words, fused = C.c_uint64(0), C.c_int32(-1)
    rc = lib.eth_kzg_amd_test_prover_scalars(ctx.handle, n, b"".join(blobs), scalars.ctypes.data, max_words, C.byref(n_words),
                                             cells.ctypes.data, proofs.ctypes.data, status.ctypes.data, C.byref(fused))
    assert rc == 0
    return scalars[:n_words.value], cells, proofs, status.tolist(), fused.value


def _both(contexts, blobs, want_words):
    a = _run(contexts["pair"], blobs)
    b = _run(contexts["fused"], blobs)
    assert a[4] == 0 and b[4] == 1, "the knob did not force the two schedules"
    assert len(a[0]) == len(b[0]) == want_words
    assert np.array_equal(a[0], b[0]), "MSM scalars differ at words %s ..." % np.flatnonzero(a[0] != b[0])[:8]
    assert a[3] == b[3]
    assert np.array_equal(a[1], b[1]), "cells differ"
    assert np.array_equal(a[2], b[2]), "proofs differ"
    return b


def _batches(n):
    """the seven inputs of the issue (a random blob and SPECIAL) as batches of n"""
    if n == 1:
        return [[_blob("random")]] + [[_blob(k)] for k in SPECIAL]
    if n == 2:
        seq = [_blob("random")] + [_blob(k) for k in SPECIAL] + [_blob("random", 1)]
        return [seq[i:i + 2] for i in range(0, 8, 2)]
    batch = [_blob("random", s) for s in range(n)]
    for pos, kind in zip((1, 7, 31, 62, 63, 64), SPECIAL):  # both sides of the lane-group boundary among them
        batch[pos] = _blob(kind)
    return [batch]


@pytest.mark.parametrize("n", [1, 2, 65])
def test_scalars_cells_and_proofs_match_the_pair_and_the_oracle(contexts, oracle, n):
    """Every word of the MSM's scalars (the segment copies of one and two blobs included), every byte of cells and proofs: fused kernel ==
    old pair; cells and proofs == the oracle for every blob that is not one of the random fill of the 65-blob batch (its first four are)."""
    segs = 4 if n <= 2 else 1
    for batch in _batches(n):
        _, cells, proofs, status, _ = _both(contexts, batch, segs * n * 8192 * 8)
        assert status == [0] * n
        check = range(n) if n <= 2 else [0, 1, 2, 3, 4, 7, 31, 62, 63, 64]
        for b in check:
            ec, ep = _expected(oracle, batch[b])
            assert cells[b].tobytes() == ec, (n, b)
            assert proofs[b].tobytes() == ep, (n, b)
            assert ec[:131072] == batch[b]


def test_a_rejected_blob_between_valid_ones(contexts, oracle):
    """n = 3, the middle blob with an element >= r: it takes the full transform (its bytes are no canonical encoding), so statuses, scalars
    and all three blobs' cells and proofs are the old pair's; the valid neighbours give the oracle's bytes."""
    bad = bytearray(_blob("random", 2))
    bad[32 * 100:32 * 101] = b"\xff" * 32
    batch = [_blob("random"), bytes(bad), _blob("e63")]
    _, cells, proofs, status, _ = _both(contexts, batch, 3 * 8192 * 8)  # three blobs take the compiled linear map: no segment copies
    assert status == [0, 1, 0]
    assert cells[1, :131072].tobytes() != bytes(bad)
    for b in (0, 2):
        ec, ep = _expected(oracle, batch[b])
        assert cells[b].tobytes() == ec and proofs[b].tobytes() == ep, b


def test_the_engine_picks_the_fused_kernel_above_the_side_stream_batches(contexts, oracle):
    """Knob unset: 65 blobs compute their cells on the second stream next to the proof stages (the pair), 300 blobs take the fused kernel;
    the same bytes as the forced pair either way, a sample against the oracle."""
    small = _batches(65)[0]
    got = _run(contexts["auto"], small)
    assert got[4] == 0
    batch = small + [_blob("random", 100 + s) for s in range(235)]
    want = _run(contexts["pair"], batch)
    got = _run(contexts["auto"], batch)
    assert want[4] == 0 and got[4] == 1
    assert np.array_equal(want[0], got[0]) and want[3] == got[3] == [0] * 300
    assert np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2])
    for b in (0, 64, 299):
        ec, ep = _expected(oracle, batch[b])
        assert got[1][b].tobytes() == ec and got[2][b].tobytes() == ep, b
