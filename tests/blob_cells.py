"""The statement of eth_kzg_amd_verify_blob_cell_proofs_many (csrc/verify_host.hpp, the blob source of the cell many-verification), in
Python -- never the library.

Item i = (blob_i, commitment C_i, [128 cell proofs]).  There is no new transcript: the item is the problem
    (128 x C_i, indices 0..127, compute_cells(blob_i), proofs_i)
of the many-verification under the leaf-hashed challenge of that problem alone (tests/many_leaf.py).  The status of an item, in the
order of checks of the reference's two calls (compute_cells, then verify_cell_kzg_proof_batch): 1 if the blob holds an element >= r
(also when a point is bad as well), else 2 if the commitment or one of the 128 proofs is not a canonical point of the subgroup, else 0.
Only items of status 0 are live.  A call is cut like any many-verification call whose problems hold 128 cells: parts from 192 items
(24576 cells) on, at most three; passes of at most 131072 / 128 = 1024 items."""
import oracle_lib
from blob_many import BLOB_BYTES, INF, R, blob_is_bad, monomial_blob, with_element  # noqa: F401

N_CELLS = 128
CELL_BYTES = 2048
MAX_ITEMS = 1 << 24
MIN_PROBLEMS, MIN_CELLS, MAX_PARTS, CHUNK = 192, 24576, 3, 131072  # csrc/engine.hpp (tests/test_vm_plan_host.py holds them to it)
PASS = CHUNK // N_CELLS


def merge(blob_bad, point_bad, passed):
    """-> (status, verified) of an item: the order of checks of the issue, written out case by case"""
    if blob_bad:
        return 1, False
    if point_bad:
        return 2, False
    return 0, bool(passed)


def item_status(item):
    blob, c, proofs = item
    if blob_is_bad(blob):
        return 1
    if oracle_lib.g1_validate(c, True) != 0 or any(oracle_lib.g1_validate(p, True) != 0 for p in set(proofs)):
        return 2
    return 0


def expand(item, cells):
    """the problem of an item, cells = compute_cells(blob) from whoever computed them: (commitments, indices, cells, proofs)"""
    _, c, proofs = item
    assert len(cells) == len(proofs) == N_CELLS
    return ([c] * N_CELLS, list(range(N_CELLS)), list(cells), list(proofs))


def blob_cells(blob):
    """cells 0..63 of a blob: its own bytes"""
    return [blob[CELL_BYTES * k:CELL_BYTES * (k + 1)] for k in range(N_CELLS // 2)]


def slice_of(i):
    """(byte offset of item i's blob, of its extension) from the first cell of a pass"""
    return 2 * i * BLOB_BYTES, (2 * i + 1) * BLOB_BYTES


def parts(n):
    """cut points of a call of n items (the rule of vm_call_parts at 128 cells per problem, written for equal problems)"""
    if n == 0:
        return [0]
    if n < MIN_PROBLEMS or n * N_CELLS < MIN_CELLS or MAX_PARTS < 2:
        return [0, n]
    cuts = [0]
    for b in range(n):
        if len(cuts) < MAX_PARTS and (b + 1) * MAX_PARTS >= n * len(cuts) and b + 1 < n:
            cuts.append(b + 1)
    return cuts + [n]


def chunks(n, chunk=CHUNK):
    per = max(1, chunk // N_CELLS)
    return list(range(0, n, per)) + [n]
