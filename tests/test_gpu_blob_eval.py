"""k_blob_eval_at alone (csrc/k_ntt.hip, through the hook eth_kzg_amd_test_blob_eval_at): y = p(z) of a blob, evaluated inside the CU.

Expected values: the CPU oracle's evaluation (the y of its compute_kzg_proof), the y of eth_kzg_amd_compute_kzg_proof_batch for the same
(blob, z) byte for byte, and the closed forms -- a point of the domain gives the element at its place, a constant blob its constant, the
monomial X^j gives z^j (so every thread's power z^(j mod 1024) and every k of the Horner step over j + 1024 k is hit alone).
One launch of the 21 well-formed cases (also as n = 1 and n = 2), and one of five refused blobs between three of the well-formed ones:
bad = 1 and y = zero bytes for the refused, nothing changes for the others."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import blob_many as BM
import synth

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu
R = BM.R
MONOMIALS = [0, 1, 31, 32, 1023, 1024, 2047, 2048, 3071, 3072, 4095]
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    saved = os.environ.get("ETH_KZG_AMD_TABLE_GB")
    os.environ["ETH_KZG_AMD_TABLE_GB"] = "3"  # the start tables: results never depend on the table
    try:
        c = kzg.DASContext(use_precomp=True)
    finally:
        if saved is None:
            os.environ.pop("ETH_KZG_AMD_TABLE_GB", None)
        else:
            os.environ["ETH_KZG_AMD_TABLE_GB"] = saved
    yield c
    c.close()


def eval_at(ctx, pairs):
    """[(blob, z int)] -> ([y bytes], [bad]) by one launch of the kernel"""
    lib = kzg.load_library()
    n = len(pairs)
    ptrs, keep = kzg._alias_ptrs([b for b, _ in pairs])
    zs = b"".join(BM.fr_be(z) for _, z in pairs)
    ys, bad = C.create_string_buffer(32 * n), (C.c_int32 * n)()
    rc = lib.eth_kzg_amd_test_blob_eval_at(ctx.handle, n, ptrs.ctypes.data_as(C.c_void_p), zs, ys, bad)
    assert rc == 0, rc
    return [ys.raw[32 * i:32 * i + 32] for i in range(n)], list(bad)


def well_formed():
    """[(name, blob, z, closed form or None)]: computed once, shared, never changed"""
    if "cases" not in _cache:
        zr = [int.from_bytes(s, "big") for s in synth.seeded_scalars(4, b"blob-eval:z")]
        blob = synth.seeded_blob(3)
        el = lambda at: int.from_bytes(blob[32 * at:32 * at + 32], "big")  # noqa: E731
        cases = [("random", blob, zr[0], None), ("z=0", blob, 0, None), ("z=1", blob, 1, el(0)), ("z=r-1", blob, R - 1, el(1))]
        for k in (1, 2048, 4095):  # omega^k: the element at brp(k) (omega^2048 = r - 1: the same point as above, by another name)
            cases.append(("z=w^%d" % k, blob, pow(BM.W4096, k, R), el(BM.brp(k, 12))))
        v = zr[1]
        cases.append(("constant", BM.blob_of([v] * BM.N), zr[2], v))
        cases.append(("all-zero", bytes(BM.BLOB_BYTES), zr[2], 0))
        cases.append(("all-r-1", BM.blob_of([R - 1] * BM.N), zr[2], R - 1))
        for j in MONOMIALS:
            cases.append(("X^%d" % j, BM.monomial_blob(j), zr[3], pow(zr[3], j, R)))
        assert len(cases) == 21
        _cache["cases"] = cases
    return _cache["cases"]


@pytest.fixture(scope="module")
def launch_a(ctx):
    return eval_at(ctx, [(b, z) for _, b, z, _ in well_formed()])


def test_well_formed_against_the_oracle_and_the_closed_forms(ctx, oracle, launch_a):
    ys, bad = launch_a
    assert bad == [0] * 21
    for (name, blob, z, closed), y in zip(well_formed(), ys):
        _, want = oracle.compute_kzg_proof(blob, BM.fr_be(z))
        assert y == want, (name, y.hex(), want.hex())
        if closed is not None:
            assert y == BM.fr_be(closed), name
    assert ys[0] == BM.fr_be(BM.blob_eval(well_formed()[0][1], well_formed()[0][2]))  # and Python integers, once


def test_equals_compute_kzg_proof_batch_byte_for_byte(ctx, launch_a):
    cases = well_formed()
    st, _, ys = ctx.compute_kzg_proof_batch([b for _, b, _, _ in cases], [BM.fr_be(z) for _, _, z, _ in cases])
    assert st == [0] * 21
    assert list(ys) == launch_a[0]


def test_launches_of_one_and_two_blobs(ctx, launch_a):
    pairs = [(b, z) for _, b, z, _ in well_formed()]
    assert eval_at(ctx, pairs[:1]) == (launch_a[0][:1], [0])
    assert eval_at(ctx, pairs[10:12]) == (launch_a[0][10:12], [0, 0])  # X^0 and X^1


def test_refused_blobs_and_their_neighbours(ctx, launch_a):
    cases = well_formed()
    blob, z = cases[0][1], cases[0][2]
    refused = [BM.with_element(blob, at, R) for at in (0, 1023, 1024, 4095)] + [BM.with_element(blob, 2000, (1 << 256) - 1)]
    keep = [0, 7, 20]  # random, constant, X^4095
    pairs, want_y, want_bad = [], [], []
    for i, rb in enumerate(refused):
        pairs.append((rb, z))
        want_y.append(bytes(32))
        want_bad.append(1)
        if i < 3:
            k = keep[i]
            pairs.append((cases[k][1], cases[k][2]))
            want_y.append(launch_a[0][k])
            want_bad.append(0)
    assert len(pairs) == 8
    assert eval_at(ctx, pairs) == (want_y, want_bad)
    assert eval_at(ctx, pairs[:1]) == ([bytes(32)], [1])
