"""The leaf-hashed Fiat-Shamir challenge of the cell verifier (ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT), stated in hashlib.

Written from the definition, not from csrc/verify_host.hpp or csrc/k_sha256.hip:

    LEAF_k = SHA-256( "RCKZGCBATCHLEAF1"            16 bytes
                    | be64(k)                        position in the caller's list
                    | be64(cell_indices[k])
                    | commitments[k]                 48 bytes, the caller's bytes for entry k (no de-duplication)
                    | proofs[k]                      48 bytes
                    | cells[k] )                     2048 bytes
    ROOT   = SHA-256( "RCKZGCBATCHROOT1" | be64(4096) | be64(64) | be64(n) | LEAF_0 | ... | LEAF_{n-1} )
    r      = ROOT as a 256-bit big-endian integer mod r

tests/test_leaf_transcript_host.py compares the host statement with it on the CPU, tests/test_gpu_leaf_transcript.py the kernel's
digests, the root the verifier hashes and, through verify_transcript.cell_partial(..., r=leaf_challenge(...)), the pairing inputs."""
import hashlib

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001  # the order of the BLS12-381 scalar field
LEAF_DOMAIN = b"RCKZGCBATCHLEAF1"
ROOT_DOMAIN = b"RCKZGCBATCHROOT1"
LEAF_MESSAGE_BYTES = 16 + 8 + 8 + 48 + 48 + 2048


def be64(v):
    return int(v).to_bytes(8, "big")


def leaf_digest(k, index, commitment, proof, cell):
    assert len(commitment) == 48 and len(proof) == 48 and len(cell) == 2048
    msg = LEAF_DOMAIN + be64(k) + be64(index) + bytes(commitment) + bytes(proof) + bytes(cell)
    assert len(msg) == LEAF_MESSAGE_BYTES == 34 * 64
    return hashlib.sha256(msg).digest()


def leaf_digests(commitments, indices, cells, proofs):
    n = len(indices)
    assert len(commitments) == len(cells) == len(proofs) == n
    return [leaf_digest(k, indices[k], commitments[k], proofs[k], cells[k]) for k in range(n)]


def root_of(leaves):
    return hashlib.sha256(ROOT_DOMAIN + be64(4096) + be64(64) + be64(len(leaves)) + b"".join(leaves)).digest()


def leaf_root(commitments, indices, cells, proofs):
    """the 32 bytes the challenge is reduced from"""
    return root_of(leaf_digests(commitments, indices, cells, proofs))


def leaf_challenge(commitments, indices, cells, proofs):
    return int.from_bytes(leaf_root(commitments, indices, cells, proofs), "big") % R
