"""The batched and device-resident EIP-4844 proof entry points (eth_kzg_amd_compute_blob_kzg_proof_batch / _device,
eth_kzg_amd_compute_kzg_proof_batch / _device, eth_kzg_amd_verify_blob_kzg_proof_batch_device) and the many-message SHA-256 kernel
under them (csrc/k_sha256.hip, through its test hook), against hashlib, the reference's golden vectors and the CPU oracle.
Bit-exact: everything here is integer / byte work.

Run on the MI355X box:  python -m pytest tests/test_gpu_eip4844_batch.py -m gpu -x -q
"""
import hashlib
import importlib
import os

import numpy as np
import pytest

import synth
import vectors

pytestmark = pytest.mark.gpu
kzg = importlib.import_module("rust-eth-kzg_amd")

BLOB = 131072
R_BYTES = synth.R.to_bytes(32, "big")


def _torch():
    # torch initialises its HIP state before the engine creates its streams (the other order has failed to find the GPU)
    import torch
    torch.cuda.init()
    return torch


@pytest.fixture(scope="module")
def ctx():
    """One context on the library's default tables: the commitment table is the only one these paths touch."""
    _torch()
    saved = os.environ.pop("ETH_KZG_AMD_TABLE_GB", None)
    c = None
    try:
        c = kzg.DASContext(use_precomp=True)
        yield c
    finally:
        if c is not None:
            c.close()
        if saved is not None:
            os.environ["ETH_KZG_AMD_TABLE_GB"] = saved


def _dev(data):
    """bytes / uint8 array -> a flat uint8 tensor in HBM (at least one byte, so that it has an address)"""
    torch = _torch()
    a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).reshape(-1)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.copy()).cuda()


def _rows(t, n, width):
    raw = t.cpu().numpy().tobytes()
    return [raw[width * i:width * (i + 1)] for i in range(n)]


def _random_blobs(n, seed):
    """n blobs of uniformly random canonical field elements (top two bits cleared: < 2^254 < r), as bytes"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, 4096, 32), dtype=np.uint8)
    a[:, :, 0] &= 0x3F
    return [a[b].tobytes() for b in range(n)]


def _blob_proofs_device(ctx, blobs, comms, **kw):
    torch = _torch()
    n = len(blobs)
    d_b, d_c = _dev(b"".join(blobs)), _dev(b"".join(comms))
    d_p = torch.zeros(max(1, n) * 48, dtype=torch.uint8, device="cuda")
    st = ctx.compute_blob_kzg_proof_device(n, d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), **kw)
    torch.cuda.synchronize()
    return st, _rows(d_p, n, 48)


def _proofs_at_device(ctx, blobs, zs):
    torch = _torch()
    n = len(blobs)
    d_b, d_z = _dev(b"".join(blobs)), _dev(b"".join(zs))
    d_p = torch.zeros(max(1, n) * 48, dtype=torch.uint8, device="cuda")
    d_y = torch.zeros(max(1, n) * 32, dtype=torch.uint8, device="cuda")
    st = ctx.compute_kzg_proof_device(n, d_b.data_ptr(), d_z.data_ptr(), d_p.data_ptr(), d_y.data_ptr())
    torch.cuda.synchronize()
    return st, _rows(d_p, n, 48), _rows(d_y, n, 32)


def _verify_device(ctx, blobs, comms, proofs):
    d_b, d_c, d_p = _dev(b"".join(blobs)), _dev(b"".join(comms)), _dev(b"".join(proofs))
    return ctx.verify_blob_kzg_proof_batch_device(len(blobs), d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr())


def _single_error_code(fn, *args):
    """the status code of the single call's error class: 1 CouldNotDeserializeScalar, 2 CouldNotDeserializeG1Point"""
    try:
        fn(*args)
    except kzg.KzgError as e:
        return {"Serialization(CouldNotDeserializeScalar)": 1, "Serialization(CouldNotDeserializeG1Point)": 2}[str(e)]
    raise AssertionError("the single call accepted an invalid case")


# ------------------------------------------------------------------ 1. the hash kernel alone
# (prefix, body, tail) lengths per total length around the padding rule: 55 is the last length whose padding fits the data's own
# block, 56 .. 63 need a block more, 64 starts a new one; 119 / 120 are the same edge one block on.
SPLITS = [
    (0, 0, 0), (0, 1, 0), (55, 0, 0), (0, 0, 56), (20, 23, 20), (0, 64, 0), (65, 0, 0), (30, 70, 19), (10, 20, 90), (70, 0, 58),
    (32, 96, 0),  # 128 again: block 1 lies wholly inside a 16-byte-aligned body -- the kernel's wide-load path at a small size
]


def test_hash_splits_cover_what_they_should():
    assert sorted({sum(s) for s in SPLITS}) == [0, 1, 55, 56, 63, 64, 65, 119, 120, 128]
    for part in range(3):
        assert any(s[part] == 0 for s in SPLITS), part  # each part empty at least once
        crosses = [s for s in SPLITS if s[part] and sum(s[:part]) // 64 != (sum(s[:part + 1]) - 1) // 64]
        assert crosses, part  # each part crosses a 64-byte block boundary at least once


def _sha_many(ctx, n, prefix, bodies, body_len, body_stride, tails, tail_len, tail_stride):
    """bodies / tails: n rows of body_len / tail_len bytes, laid out with the given strides; returns the n digests"""
    torch = _torch()
    lib = kzg.load_library()
    body = np.zeros(max(1, n * body_stride), dtype=np.uint8)
    tail = np.zeros(max(1, n * tail_stride), dtype=np.uint8)
    for i in range(n):
        body[i * body_stride:i * body_stride + body_len] = np.frombuffer(bodies[i], dtype=np.uint8)
        tail[i * tail_stride:i * tail_stride + tail_len] = np.frombuffer(tails[i], dtype=np.uint8)
    d_body, d_tail = _dev(body), _dev(tail)
    d_out = torch.zeros(32 * n + 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = lib.eth_kzg_amd_test_sha256_many(ctx.handle, n, prefix, len(prefix), d_body.data_ptr() if body_len else None, body_stride, body_len,
                                          d_tail.data_ptr() if tail_len else None, tail_stride, tail_len, d_out.data_ptr())
    assert rc == 0
    out = d_out.cpu().numpy().tobytes()
    assert out[32 * n:] == bytes(32), "a padding lane stored a digest"
    return [out[32 * i:32 * i + 32] for i in range(n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sha256_many_around_the_padding_rule(ctx, n):
    rng = np.random.RandomState(4844 + n)
    for (pl, bl, tl) in SPLITS:
        prefix = rng.randint(0, 256, size=pl, dtype=np.uint8).tobytes()
        bodies = [rng.randint(0, 256, size=bl, dtype=np.uint8).tobytes() for _ in range(n)]
        tails = [rng.randint(0, 256, size=tl, dtype=np.uint8).tobytes() for _ in range(n)]
        # odd strides put most rows at odd addresses (the byte-gather path); 96-byte bodies keep theirs 16-byte aligned
        bs, ts = (bl if bl == 96 else bl + 3), tl + 1
        got = _sha_many(ctx, n, prefix, bodies, bl, bs, tails, tl, ts)
        for i in range(n):
            assert got[i] == hashlib.sha256(prefix + bodies[i] + tails[i]).digest(), (n, (pl, bl, tl), i)


def test_sha256_many_at_the_product_shape(ctx):
    """65 blob-sized messages (32 + 131072 + 48 bytes: 2050 blocks each) with the rows further apart than they are long"""
    n, stride = 65, BLOB + 64
    rng = np.random.RandomState(65)
    prefix = b"FSBLOBVERIFY_V1_" + (4096).to_bytes(16, "big")
    body = rng.randint(0, 256, size=(n, BLOB), dtype=np.uint8)
    bodies = [body[i].tobytes() for i in range(n)]
    tails = [rng.randint(0, 256, size=48, dtype=np.uint8).tobytes() for _ in range(n)]
    got = _sha_many(ctx, n, prefix, bodies, BLOB, stride, tails, 48, 48)
    for i in range(n):
        assert got[i] == hashlib.sha256(prefix + bodies[i] + tails[i]).digest(), i


# ------------------------------------------------------------------ 2. golden vectors, one call per family and form
def test_compute_blob_kzg_proof_vectors_in_one_call(ctx):
    cases = [c for _, c in sorted(vectors.load("compute_blob_kzg_proof").items())
             if len(c["input"]["blob"]) == BLOB and len(c["input"]["commitment"]) == 48]  # fixed-length buffers: nothing else crosses the ABI
    valid = [c["output"] is not None for c in cases]
    assert (len(cases), sum(valid)) == (11, 7)
    blobs, comms = [c["input"]["blob"] for c in cases], [c["input"]["commitment"] for c in cases]
    want_st = [0 if v else _single_error_code(ctx.compute_blob_kzg_proof, b, c) for v, b, c in zip(valid, blobs, comms)]
    assert sorted(set(want_st)) == [0, 1, 2]
    for st, proofs in (ctx.compute_blob_kzg_proof_batch(blobs, comms), _blob_proofs_device(ctx, blobs, comms)):
        assert st == want_st
        for k, c in enumerate(cases):
            if valid[k]:
                assert proofs[k] == c["output"], k


def test_compute_kzg_proof_vectors_in_one_call(ctx):
    cases = [c for _, c in sorted(vectors.load("compute_kzg_proof").items()) if len(c["input"]["blob"]) == BLOB and len(c["input"]["z"]) == 32]
    valid = [c["output"] is not None for c in cases]
    assert (len(cases), sum(valid)) == (48, 42)
    blobs, zs = [c["input"]["blob"] for c in cases], [c["input"]["z"] for c in cases]
    want_st = [0 if v else _single_error_code(ctx.compute_kzg_proof, b, z) for v, b, z in zip(valid, blobs, zs)]
    for st, proofs, ys in (ctx.compute_kzg_proof_batch(blobs, zs), _proofs_at_device(ctx, blobs, zs)):
        assert st == want_st
        for k, c in enumerate(cases):
            if valid[k]:
                assert [proofs[k], ys[k]] == list(c["output"]), k


# ------------------------------------------------------------------ 3. the batch verifier's vectors through the device form
def test_verify_blob_kzg_proof_batch_vectors_on_the_device(ctx):
    seen = 0
    for name, c in sorted(vectors.load("verify_blob_kzg_proof_batch").items()):
        i = c["input"]
        if not (len(i["blobs"]) == len(i["commitments"]) == len(i["proofs"]) and all(len(b) == BLOB for b in i["blobs"])
                and all(len(x) == 48 for x in i["commitments"] + i["proofs"])):
            continue  # one count and fixed-length buffers: nothing else crosses the device ABI
        seen += 1
        try:
            got = _verify_device(ctx, i["blobs"], i["commitments"], i["proofs"])
        except kzg.KzgError as e:
            got = None
            with pytest.raises(kzg.KzgError) as host:  # an Err of the same class as the host form's
                ctx.verify_blob_kzg_proof_batch(i["blobs"], i["commitments"], i["proofs"])
            assert str(host.value) == str(e), name
        assert got == c["output"], name
    assert seen == 15


# ------------------------------------------------------------------ 4. seeded blobs against the oracle
@pytest.fixture(scope="module")
def seeded(ctx, oracle):
    blobs = [synth.seeded_blob(4844 + i) for i in range(65)]
    st, comms = ctx.blob_to_kzg_commitment_batch(blobs)
    assert st == [0] * 65
    return blobs, comms, [oracle.compute_blob_kzg_proof(b, c) for b, c in zip(blobs, comms)]


@pytest.mark.parametrize("n", [1, 3, 64, 65])
def test_blob_proofs_of_seeded_blobs_match_the_oracle(ctx, seeded, n):
    blobs, comms, want = (x[:n] for x in seeded)
    assert ctx.compute_blob_kzg_proof_batch(blobs, comms) == ([0] * n, want)
    assert _blob_proofs_device(ctx, blobs, comms) == ([0] * n, want)


# ------------------------------------------------------------------ 5. consistency past the 256-blob host sub-batch
def test_300_blobs_both_forms_agree_and_verify(ctx, oracle):
    n = 300
    blobs = _random_blobs(n, 300)
    st, comms = ctx.blob_to_kzg_commitment_batch(blobs)
    assert st == [0] * n
    st_h, proofs = ctx.compute_blob_kzg_proof_batch(blobs, comms)
    st_d, proofs_d = _blob_proofs_device(ctx, blobs, comms)
    assert st_h == st_d == [0] * n and proofs == proofs_d
    for b in (0, 255, 256, 299):  # both sides of the cut against the oracle
        assert proofs[b] == oracle.compute_blob_kzg_proof(blobs[b], comms[b]), b
    torch = _torch()
    d_b, d_c = _dev(b"".join(blobs)), _dev(b"".join(comms))

    def verify(cm, pr):
        d_c.copy_(torch.from_numpy(np.frombuffer(b"".join(cm), dtype=np.uint8).copy()))
        d_p = _dev(b"".join(pr))
        return ctx.verify_blob_kzg_proof_batch_device(n, d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr())

    assert verify(comms, proofs) is True
    swapped = list(proofs)
    swapped[170], swapped[171] = swapped[171], swapped[170]
    assert verify(comms, swapped) is False
    broken = list(comms)
    broken[12] = bytes([broken[12][0] & 0x7F]) + broken[12][1:]  # the compression flag cleared: no longer decodes
    with pytest.raises(kzg.KzgError, match="CouldNotDeserializeG1Point"):
        verify(broken, proofs)


# ------------------------------------------------------------------ 6. a mixed batch
def test_mixed_batch_flags_each_bad_slot_and_leaves_its_neighbours_exact(ctx, seeded, oracle):
    blobs, comms = list(seeded[0][:7]), list(seeded[1][:7])
    want = list(seeded[2][:7])
    bad_blob = blobs[1][:32 * 77] + b"\xff" * 32 + blobs[1][32 * 78:]
    off_curve = vectors.load("compute_blob_kzg_proof")["invalid_commitment_1a68c47b68148e78"]["input"]["commitment"]
    assert _single_error_code(ctx.compute_blob_kzg_proof, blobs[3], off_curve) == 2
    blobs[1] = bad_blob
    comms[3] = off_curve
    blobs[5], comms[5] = bad_blob, off_curve  # both wrong: the blob's own check comes first
    want_st = [0, 1, 0, 2, 0, 1, 0]
    for st, proofs in (ctx.compute_blob_kzg_proof_batch(blobs, comms), _blob_proofs_device(ctx, blobs, comms)):
        assert st == want_st
        assert [proofs[k] for k in (0, 2, 4, 6)] == [want[k] for k in (0, 2, 4, 6)]
    # compute_kzg_proof: a bad blob, a z >= r, both
    blobs = list(seeded[0][:7])
    zs = synth.seeded_scalars(7, b"z-mixed")
    exact = {k: oracle.compute_kzg_proof(blobs[k], zs[k]) for k in (0, 2, 3, 5, 6)}
    blobs[1] = bad_blob
    zs[4] = R_BYTES
    assert _single_error_code(ctx.compute_kzg_proof, blobs[4], zs[4]) == 1
    want_st = [0, 1, 0, 0, 1, 0, 0]
    for st, proofs, ys in (ctx.compute_kzg_proof_batch(blobs, zs), _proofs_at_device(ctx, blobs, zs)):
        assert st == want_st
        for k, (p, y) in exact.items():
            assert (proofs[k], ys[k]) == (p, y), k


# ------------------------------------------------------------------ 7. asynchronous device call
def test_async_call_is_ordered_behind_the_kernel_that_writes_the_blobs(ctx, seeded):
    """status = None on the caller's stream: the call returns without synchronising and must read d_blobs only after the work the
    caller has queued on that stream -- a long kernel, then the copy that produces the blobs -- has run."""
    torch = _torch()
    n = 20
    blobs, comms, want = (x[:n] for x in seeded)
    src = _dev(b"".join(blobs))
    d_c = _dev(b"".join(comms))
    d_b = torch.zeros(n * BLOB, dtype=torch.uint8, device="cuda")
    d_p = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
    busy = torch.zeros(1 << 30, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(16):
            busy.add_(1)  # a few milliseconds of queued work in front of the copy
        d_b.copy_(src, non_blocking=True)
        assert ctx.compute_blob_kzg_proof_device(n, d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), want_status=False,
                                                 stream=stream.cuda_stream) is None
    stream.synchronize()
    assert _rows(d_p, n, 48) == want
    # and with NULL for the stream: ordered behind the default stream, synchronised before it returns
    d_b.zero_()
    d_p.zero_()
    d_b.copy_(src, non_blocking=True)
    ctx.compute_blob_kzg_proof_device(n, d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), want_status=False)
    assert _rows(d_p, n, 48) == want


# ------------------------------------------------------------------ 8. device-list context
def test_device_list_context_gives_the_same_bytes(ctx, seeded):
    blobs, comms, want = (x[:5] for x in seeded)  # 5 blobs over two engines: slices of 2 and 3
    zs = synth.seeded_scalars(5, b"z-list")
    saved = os.environ.pop("ETH_KZG_AMD_TABLE_GB", None)
    multi = None
    try:
        multi = kzg.DASContext(use_precomp=True, devices=[0, 0])
        assert multi.devices() == [0, 0]
        assert multi.compute_blob_kzg_proof_batch(blobs, comms) == ([0] * 5, want)
        assert multi.compute_kzg_proof_batch(blobs, zs) == ctx.compute_kzg_proof_batch(blobs, zs)
        assert multi.compute_blob_kzg_proof_batch([], []) == ([], [])
        # device calls are routed by pointer to the engine that owns the buffers
        assert _blob_proofs_device(multi, blobs, comms) == ([0] * 5, want)
        assert _proofs_at_device(multi, blobs, zs) == _proofs_at_device(ctx, blobs, zs)
        assert _verify_device(multi, blobs, comms, want) is True
        assert _verify_device(multi, blobs, comms, want[::-1]) is False
        assert _verify_device(multi, [], [], []) is True
    finally:
        if multi is not None:
            multi.close()
        if saved is not None:
            os.environ["ETH_KZG_AMD_TABLE_GB"] = saved
