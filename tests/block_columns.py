"""A block's cells and proofs in the two layouts, as plain Python lists: blob-major [blob][128], what compute_cells_and_kzg_proofs_batch
and recover_cells_and_kzg_proofs_batch speak, and column-major [column][blob], what eth_kzg_amd_compute_data_columns /
_recover_data_columns / _verify_data_columns speak.  Calls no library function: the tests state the column calls' contract with it."""

CELLS = 128


def to_columns(by_blob):
    """[blob][k] -> [k][blob] (k over the cells of a blob, or over any equal-length rows)"""
    if not by_blob:
        return []
    width = len(by_blob[0])
    assert all(len(row) == width for row in by_blob)
    return [[row[k] for row in by_blob] for k in range(width)]


def to_blobs(by_column):
    """[k][blob] -> [blob][k]: the inverse of to_columns (the transpose is its own inverse)"""
    return to_columns(by_column)


def cut_columns(by_column, column_indices):
    """the columns a supernode holds: [c][blob] over all 128 -> [j][blob] over the given indices, in their order"""
    return [by_column[c] for c in column_indices]


def expand_recovery(column_indices, cells):
    """A column recovery (column_indices[j], cells[j][i]) as the batch recover_cells_and_kzg_proofs_batch takes: one
    (cell_indices, cells) list per blob -- every blob with the same indices, blob i with cells[0][i] .. cells[n_columns-1][i]."""
    n_blobs = len(cells[0]) if cells else 0
    assert all(len(col) == n_blobs for col in cells) and len(cells) == len(column_indices)
    return [(list(column_indices), [cells[j][i] for j in range(len(column_indices))]) for i in range(n_blobs)]


def index_list_status(column_indices):
    """0, or 3 for a list recover_cells_and_kzg_proofs refuses: fewer than 64 or more than 128 entries, not strictly ascending, an index >= 128"""
    idx = list(column_indices)
    if not CELLS // 2 <= len(idx) <= CELLS:
        return 3
    if any(not 0 <= c < CELLS for c in idx):
        return 3
    if any(not a < b for a, b in zip(idx, idx[1:])):
        return 3
    return 0


def flat(by_column):
    """[c][blob] byte strings -> the bytes of the device form's [c][n_blobs][size] array"""
    return b"".join(b"".join(col) for col in by_column)


def unflat(raw, n_columns, n_blobs, size):
    """the inverse of flat"""
    assert len(raw) == n_columns * n_blobs * size
    return [[raw[(c * n_blobs + i) * size:(c * n_blobs + i + 1) * size] for i in range(n_blobs)] for c in range(n_columns)]
