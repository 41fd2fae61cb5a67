"""The many-verification with leaf-hashed challenges (eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex / _many_device_ex with
ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT), stated in hashlib and Python integers; no library call.

Per problem of a pass, exactly what the single flagged call takes for that problem alone (tests/leaf_transcript.py): the leaves hash
the position INSIDE the problem, the root carries the problem's own n, and r = ROOT mod r.  Behind the challenge everything is the
unflagged pass's (tests/verify_transcript.py): the pair cell_partial(..., 0, n, r), the weights fold_weights(roots, live) -- the roots
stand where the reference transcript's digests stand, 32 zero bytes for a problem that is empty or refused at validation -- fold_pair
and search_plan as they are.

flat_arrays() builds what the device-resident form takes from a list of problems: cell_starts and the four flat arrays."""
import leaf_transcript as L
import verify_transcript as T

ZERO32 = bytes(32)


def problem_leaves(args):
    """the leaf digests of one problem: positions restart at 0"""
    return L.leaf_digests(*args)


def problem_root(args):
    return L.root_of(problem_leaves(args))


def pass_digests(problems, hashed):
    """problems[b] = (commitments, indices, cells, proofs); hashed[b]: the problem holds cells and passed validation -> the 32 bytes each
    challenge is reduced from"""
    return [problem_root(a) if on else ZERO32 for a, on in zip(problems, hashed)]


def pass_leaves(problems, hashed):
    """the leaf digests of every cell of the call in the caller's order; 32 zero bytes for the cells of an unhashed problem"""
    out = []
    for a, on in zip(problems, hashed):
        out += problem_leaves(a) if on else [ZERO32] * len(a[1])
    return out


def pass_statement(problems, hashed, live, folded):
    """-> (digests[B], sums[B] (None where the problem takes no part), rho[B], the folded pair or None)"""
    digests = pass_digests(problems, hashed)
    sums = [T.cell_partial(*a, 0, len(a[1]), r=T.reduce_digest(d)) if on else None for a, d, on in zip(problems, digests, live)]
    rho = T.fold_weights(digests, live)
    return digests, sums, rho, (T.fold_pair(sums, rho, 0, len(sums)) if folded else None)


def flat_arrays(problems):
    """-> (cell_starts, commitments, indices, cells, proofs): n_batches + 1 starts and the four columns of all problems back to back
    (lists; the caller joins the bytes).  The four lengths of a problem must be equal: the flat form has one length per problem."""
    starts, comm, idx, cells, proofs = [0], [], [], [], []
    for c, i, l, p in problems:
        assert len(c) == len(i) == len(l) == len(p)
        comm += c
        idx += i
        cells += l
        proofs += p
        starts.append(len(idx))
    return starts, comm, idx, cells, proofs
