"""Partial data columns (eth_kzg_amd_verify_partial_data_columns / _device) as problems of the many-verification; no library call.

A partial call is (commitments[n_blobs], column_indices[n_columns], present[n_columns], cells[n_columns][m_j], proofs[n_columns][m_j]):
present[j] is a Python int whose bit i says that column j carries blob i, and cells[j][k] / proofs[j][k] belong to the k-th set bit in
ascending blob order.  Column j IS the problem (commitments[i] for the set bits i, m_j copies of column_indices[j], cells[j], proofs[j])
of eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex: there is no new transcript, so every digest, leaf, pair, weight, fold and probe of
a partial pass is what tests/verify_transcript.py / tests/many_leaf.py state for expand(...)."""
N_CELLS = 128
MAX_BLOBS = (1 << 24) - 1


def words(n_blobs):
    return (n_blobs + 63) // 64


def blobs_of(n_blobs, present):
    """the blobs a column carries, ascending: the set bits below n_blobs"""
    return [i for i in range(n_blobs) if (present >> i) & 1]


def entries_of(n_blobs, present):
    """the entries a column occupies in the packed device arrays: the set bits of ALL its W words, stray bits included"""
    return bin(present & ((1 << (64 * words(n_blobs))) - 1)).count("1")


def validation_status(n_blobs, column_index, present):
    """3 for more blobs than a problem may hold (nothing read), a set bit at or beyond n_blobs, or cells under an index >= 128"""
    if n_blobs > MAX_BLOBS:
        return 3
    if present >> n_blobs:
        return 3
    return 3 if present and column_index >= N_CELLS else 0


def expand(commitments, column_indices, present, cells, proofs):
    """-> the problems [(commitments, indices, cells, proofs)] of the many-verification, one per column that validation accepts (None
    in the place of a refused one)"""
    nb = len(commitments)
    assert len(cells) == len(proofs) == len(column_indices) == len(present)
    out = []
    for j, c in enumerate(column_indices):
        if validation_status(nb, c, present[j]):
            out.append(None)
            continue
        held = blobs_of(nb, present[j])
        assert len(cells[j]) == len(proofs[j]) == len(held), j
        out.append(([commitments[i] for i in held], [c] * len(held), list(cells[j]), list(proofs[j])))
    return out


def mask(dense_call, present):
    """a dense column call (tests/data_columns.py: commitments, indices, cells[j][i], proofs[j][i]) under bitmaps -> the partial call;
    stray bits keep their place in the bitmap and bring no cells"""
    comm, indices, cells, proofs = dense_call
    nb = len(comm)
    pick = lambda col, p: [col[i] for i in blobs_of(nb, p)]  # noqa: E731
    return (list(comm), list(indices), list(present), [pick(cells[j], p) for j, p in enumerate(present)],
            [pick(proofs[j], p) for j, p in enumerate(present)])


def flat_bytes(call, filler=b"\xee"):
    """-> (commitments, cells, proofs) as the device form's three byte arrays: [n_blobs][48], [N][2048], [N][48], packed column after
    column; a column takes entries_of entries -- those of its stray bits, which are never read, hold `filler` bytes behind its cells"""
    comm, _, present, cells, proofs = call
    nb = len(comm)
    dc, dp = [], []
    for j, p in enumerate(present):
        stray = entries_of(nb, p) - len(cells[j])
        assert stray >= 0
        dc += list(cells[j]) + [filler * 2048] * stray
        dp += list(proofs[j]) + [filler * 48] * stray
    return b"".join(comm), b"".join(dc), b"".join(dp)


def word_rows(n_blobs, present):
    """the bitmaps as the C ABI takes them: per column W little-end-first 64-bit words"""
    return [[(p >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(words(n_blobs))] for p in present]


def dedup(items):
    """first-occurrence order -> (unique list, row of every entry): deduplicate_with_indices"""
    uniq, row = [], []
    for x in items:
        if x not in uniq:
            uniq.append(x)
        row.append(uniq.index(x))
    return uniq, row


def pairs(commitments, present_blobs):
    """the (column, commitment) pairs of one column: its own unique list as indices into the CALL's unique list, and its cells' rows
    re-ranked inside it -> (pair_u, own rows, pass-wide rows)"""
    call_uniq, call_row = dedup(commitments)
    pair_u, own = [], []
    for i in present_blobs:
        if call_row[i] not in pair_u:
            pair_u.append(call_row[i])
        own.append(pair_u.index(call_row[i]))
    return pair_u, own, [call_row[i] for i in present_blobs]


def counts(commitments, column_indices, present):
    """-> (commitment points a pass decodes, scalar multiplications of decoded points it launches) for a call that is one pass: the
    call's unique commitments once, and n + P + Bc -- n cells, P pairs, one h^64 A per column -- where the dense addressing would
    launch n + Bc n_u + Bc and the expanded pass 2 n + P"""
    nb = len(commitments)
    n = sum(len(blobs_of(nb, p)) for p in present)
    n_pairs = sum(len(pairs(commitments, blobs_of(nb, p))[0]) for p in present)
    return len(set(commitments)), n + n_pairs + len(column_indices)
