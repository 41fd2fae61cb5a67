"""Run by tests/test_gpu_parity.py in a process of its own with ETH_KZG_AMD_COOP_POINTS=0 (the limit is read once per process):
the one-lane-per-point forms of the verification kernels -- which small inputs no longer reach by default -- on the
single path, a small many-verification pass and the EIP-4844 verifier, valid, tampered and with the small-order points of
tests/small_order.py planted as proof and as commitment, then every off-subgroup case and the identity in ONE short-chain pass
(k_vm_products<VmLane>'s one-lane subgroup blocks; the form is asserted); and the prover's G1 stage with a lane per
blob where twelve blobs would take four (eth_kzg_amd_test_proofs_from_sums on the planned degenerate lanes of tests/linmap_model.py)."""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
kzg = importlib.import_module("rust-eth-kzg_amd")


def main():
    rng = np.random.RandomState(5)
    nb = 3
    blobs = rng.randint(0, 256, size=(nb, 4096, 32), dtype=np.uint8)
    blobs[:, :, 0] &= 0x3F
    blobs = [blobs[i].tobytes() for i in range(nb)]
    ctx = kzg.DASContext(True)
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(blobs)
    assert st == [0] * nb
    _, comms = ctx.blob_to_kzg_commitment_batch(blobs)
    probs = [([comms[b]] * 128, list(range(128)), cells[b], proofs[b]) for b in range(nb)]
    bad = list(proofs[1]); bad[7] = proofs[0][7]
    tampered = ([comms[1]] * 128, list(range(128)), cells[1], bad)
    assert ctx.verify_cell_kzg_proof_batch(*probs[0]) is True
    assert ctx.verify_cell_kzg_proof_batch(*tampered) is False
    ver, stt = ctx.verify_cell_kzg_proof_batch_many([probs[0], tampered, probs[2]])
    assert stt == [0, 0, 0] and ver == [True, False, True], (ver, stt)
    # a proof that is a curve point OUTSIDE the subgroup (the oracle confirms: on the curve, rejected with the subgroup test): an error
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oracle_lib
    x = 5
    while True:
        cand = bytearray(x.to_bytes(48, "big")); cand[0] |= 0x80
        if oracle_lib.g1_validate(bytes(cand), False) == 0 and oracle_lib.g1_validate(bytes(cand), True) != 0:
            break
        x += 1
    p2 = list(proofs[0]); p2[3] = bytes(cand)
    try:
        ctx.verify_cell_kzg_proof_batch([comms[0]] * 128, list(range(128)), cells[0], p2)
        raise AssertionError("a proof outside the subgroup was accepted as input")
    except kzg.KzgError:
        pass
    ver, stt = ctx.verify_cell_kzg_proof_batch_many([probs[0], ([comms[0]] * 128, list(range(128)), cells[0], p2)])
    assert stt[0] == 0 and ver[0] is True and stt[1] != 0, (ver, stt)
    z = (12345).to_bytes(32, "big")
    proof, y = ctx.compute_kzg_proof(blobs[0], z)
    assert ctx.verify_kzg_proof(comms[0], z, y, proof) is True
    assert ctx.verify_kzg_proof(comms[1], z, y, proof) is False
    # the planned points of tests/small_order.py -- small order, and a subgroup point plus a small-order point -- as proof and as
    # commitment: the one-lane subgroup tests (k_pip_shift_subgroup's branch, k_g1_decompress; the many-verification in whichever form
    # the host's thread count gives this pass) refuse them, and the problems next to them keep their verdicts
    import small_order
    bproof = ctx.compute_blob_kzg_proof(blobs[0], comms[0])
    assert ctx.verify_blob_kzg_proof(blobs[0], comms[0], bproof) is True
    for l in small_order.G1_PRIMES:
        for mixed in (False, True):
            case = small_order.planted(l, mixed)
            assert case.status1 == 2
            for role in ("proof", "commitment"):
                pl, cl = list(proofs[0]), [comms[0]] * 128
                (pl if role == "proof" else cl)[77] = case.enc
                try:
                    ctx.verify_cell_kzg_proof_batch(cl, list(range(128)), cells[0], pl)
                    raise AssertionError("%s accepted as %s" % (case.name, role))
                except kzg.KzgError as e:
                    assert "CouldNotDeserializeG1Point" in str(e), (case.name, role, e)
                ver, stt = ctx.verify_cell_kzg_proof_batch_many([probs[0], (cl, list(range(128)), cells[0], pl), tampered, probs[2]])
                assert stt == [0, 2, 0, 0] and ver == [True, False, False, True], (case.name, role, ver, stt)
                for args in ((case.enc, z, y, proof) if role == "commitment" else (comms[0], z, y, case.enc),):
                    try:
                        ctx.verify_kzg_proof(*args)
                        raise AssertionError("%s accepted as %s by verify_kzg_proof" % (case.name, role))
                    except kzg.KzgError as e:
                        assert "CouldNotDeserializeG1Point" in str(e), (case.name, role, e)
                try:
                    ctx.verify_blob_kzg_proof(blobs[0], case.enc if role == "commitment" else comms[0], case.enc if role == "proof" else bproof)
                    raise AssertionError("%s accepted as %s by verify_blob_kzg_proof" % (case.name, role))
                except kzg.KzgError as e:
                    assert "CouldNotDeserializeG1Point" in str(e), (case.name, role, e)
    assert ctx.verify_cell_kzg_proof_batch(*probs[0]) is True
    # k_vm_products<VmLane>'s one-lane subgroup blocks on EVERY off-subgroup case, the identity and valid controls in one pass
    # (small_order.many_plan): a context with eight helper threads, so that twelve problems are a short-chain pass on any machine
    from many_coop_off_check import many_sums
    os.environ["ETH_KZG_AMD_HOST_THREADS"] = "8"
    c8 = kzg.DASContext(True)
    valid = [([comms[b % 2]] * 8, list(range(8 * (b // 2), 8 * (b // 2) + 8)), cells[b % 2][8 * (b // 2):8 * (b // 2) + 8],
              proofs[b % 2][8 * (b // 2):8 * (b // 2) + 8]) for b in range(12)]
    base, planted = small_order.many_plan(valid)
    rc, ref = many_sums(c8, base)
    assert rc == 0 and ref.small and ref.status == [0] * 12 and ref.verified == [b not in (7, 9) for b in range(12)], (rc, ref.small, ref.status, ref.verified)
    rc, got = many_sums(c8, planted)
    assert rc == 0 and got.small and not got.folded, (rc, got.small, got.folded)
    assert got.status == small_order.MANY_STATUS and got.verified == small_order.MANY_VERDICTS, (got.status, got.verified)
    live = [b for b in range(12) if b not in small_order.MANY_PLANTED]
    assert [got.sums[b] for b in live] == [ref.sums[b] for b in live]
    assert c8.verify_cell_kzg_proof_batch_many(planted) == (got.verified, got.status)
    c8.close()
    # the linear map's one-lane-per-blob kernels on twelve lanes (k_slp_mulc_s, k_slp_add_s: with the quad kernels on, twelve blobs
    # never reach them): program 2 on its planned degenerate, generic and all-identity lanes, byte for byte against the definition
    import g1_stage_cases
    for k, (batch, vectors) in enumerate(g1_stage_cases.linmap_batches(2, 12)):
        g1_stage_cases.check_linmap_batch(kzg.load_library(), ctx.handle, 2, 2, 12, batch, vectors, seed=1000 * 2 + 10 * 12 + k)
    ctx.close()
    print("coop-off ok")


if __name__ == "__main__":
    main()
