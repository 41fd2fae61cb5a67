"""The data columns of one block (eth_kzg_amd_verify_data_columns / _device) as problems of the many-verification; no library call.

A column call is (commitments[n_blobs], column_indices[n_columns], cells[n_columns][n_blobs], proofs[n_columns][n_blobs]).  Column j IS
the problem (commitments as given, n_blobs copies of column_indices[j], cells[j], proofs[j]) of
eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex: there is no new transcript, so every digest, leaf, pair, weight, fold and probe of a
column pass is what tests/verify_transcript.py / tests/many_leaf.py state for expand(...)."""
N_CELLS = 128
MAX_BLOBS = (1 << 24) - 1


def expand(commitments, column_indices, cells, proofs):
    """-> the problems [(commitments, indices, cells, proofs)] of the many-verification, one per column"""
    assert len(cells) == len(proofs) == len(column_indices)
    assert all(len(c) == len(commitments) for c in cells) and all(len(p) == len(commitments) for p in proofs)
    return [(list(commitments), [c] * len(commitments), list(cells[j]), list(proofs[j])) for j, c in enumerate(column_indices)]


def block(commitments, all_cells, all_proofs, picks, column_indices):
    """the column call of a block whose blob i is material blob picks[i] (commitments[b], all_cells[b][128], all_proofs[b][128]); a
    column index >= 128 gets the cells and proofs of column 0 (it is refused before they are looked at)"""
    at = [c if c < N_CELLS else 0 for c in column_indices]
    return ([commitments[b] for b in picks], list(column_indices), [[all_cells[b][c] for b in picks] for c in at],
            [[all_proofs[b][c] for b in picks] for c in at])


def validation_status(n_blobs, column_index):
    """what validation says of one column: 3 for more blobs than a problem may hold or, in a column that holds cells, an index >= 128"""
    if n_blobs > MAX_BLOBS:
        return 3
    return 3 if n_blobs and column_index >= N_CELLS else 0


def flat_bytes(commitments, cells, proofs):
    """-> (commitments, cells, proofs) as the device form's three byte arrays: [n_blobs][48], [n_columns][n_blobs][2048], [..][48]"""
    return b"".join(commitments), b"".join(c for col in cells for c in col), b"".join(p for col in proofs for p in col)


def counts(n_cells, n_columns_in_pass, n_unique):
    """-> (commitment points a pass decodes, scalar multiplications of decoded points it launches): n_u and n + Bc n_u + Bc for the n
    cells of the Bc columns of the pass (a column refused at validation holds no cells), where the expanded pass decodes Bc n_u
    commitments and launches 2 n + Bc n_u"""
    return n_unique, n_cells + n_columns_in_pass * n_unique + n_columns_in_pass
