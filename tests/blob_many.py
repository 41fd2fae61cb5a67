"""The statement of eth_kzg_amd_verify_blob_kzg_proof_many (csrc/verify_host.hpp, the blob source of the point many-verification), in
hashlib and Python integers -- never the library.

Item i = (blob_i, commitment C_i, proof pi_i).  There is no new transcript: the item becomes the point item (C_i, z_i, y_i, pi_i) of
tests/point_many.py with
    z_i = SHA-256("FSBLOBVERIFY_V1_" | be128(4096) | blob_i | C_i) mod r     from the caller's bytes as they stand
    y_i = p_i(z_i), 32 canonical big-endian bytes; 32 zero bytes if the blob is refused
and a call is cut into passes of at most PASS items.  The status of an item, in the single call's order of checks: 1 if the blob holds
an element >= r (also when a point is bad as well), else 2 if the commitment or the proof is not a canonical point of the subgroup, else
0.  Only items of status 0 are live."""
import hashlib

import oracle_lib
import point_many as PM
import synth
from verify_transcript import INF, blob_challenge, blob_eval, brp, fr_be  # noqa: F401

R = synth.R
N = 4096
BLOB_BYTES = 32 * N
PASS = 256  # the product's pass size of the blob source (csrc/verify_host.hpp: BLOB_MANY_PASS); the tests that depend on it say so
MAX_ITEMS = 1 << 24
W4096 = pow(7, (R - 1) // N, R)


def merge(blob_bad, commitment_status, proof_status, passed):
    """-> (status, live, verified) of an item: the order of checks of the issue, written out case by case"""
    if blob_bad:
        return 1, False, False
    if commitment_status != 0:
        return 2, False, False
    if proof_status != 0:
        return 2, False, False
    return 0, True, bool(passed)


def blob_is_bad(blob):
    return any(int.from_bytes(blob[32 * j:32 * j + 32], "big") >= R for j in range(N))


def item_status(item):
    blob, c, p = item
    if blob_is_bad(blob):
        return 1
    if oracle_lib.g1_validate(c, True) != 0 or oracle_lib.g1_validate(p, True) != 0:
        return 2
    return 0


def point_item(item, y=None):
    """(C, z, y, pi) of an item; y: the evaluation as 32 bytes from whoever computed it (None: Python integers, zero for a refused blob)"""
    blob, c, p = item
    z = blob_challenge(blob, c)
    if y is None:
        y = bytes(32) if blob_is_bad(blob) else fr_be(blob_eval(blob, z))
    return (c, fr_be(z), y, p)


def blob_of(values):
    assert len(values) == N
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def seeded_cheap_blob(tag):
    """4096 elements below 2^248 from SHA-256 (what tests/c/test_blob_many.cpp builds from the same 8-byte tag)"""
    assert len(tag) == 8
    return b"".join(b"\0" + hashlib.sha256(tag + i.to_bytes(8, "big")).digest()[1:] for i in range(N))


def monomial_blob(j):
    """X^j as evaluations in the blob's order: element i = omega^(brp(i) j)"""
    return blob_of([pow(W4096, brp(i, 12) * j % N, R) for i in range(N)])


def with_element(blob, position, value):
    return blob[:32 * position] + int(value).to_bytes(32, "big") + blob[32 * position + 32:]


def call_statement(items, statuses, ys, pass_size=PASS):
    """-> (bounds, [PM.PassStatement per pass], point items): the point path's statement over (C, z, y, pi)"""
    pts = [point_item(it, y) for it, y in zip(items, ys)]
    bounds, passes = PM.call_statement(pts, statuses, pass_size)
    return bounds, passes, pts
