"""The Reed-Solomon decoder's stages in plain Python integers (tests/test_rs_reference.py validates this file against the CPU
oracle without a GPU; tests/test_gpu_rs_decode.py compares the decoder's kernels with it).  No numpy, no project code.

A blob's polynomial p (degree < 4096) is evaluated on the 8192 powers of w = omega_8192; the ABI serialises the evaluations in
bit-reversed order and cuts them into 128 cells of 64: element j of cell c is p(w^brp13(64 c + j)) = p(h_c * omega_64^brp6(j)) with
h_c = w^brp7(c).  So h_c^64 = omega_128^brp7(c), the "domain index" of cell c is brp7(c), and the vanishing polynomial of a set of
missing cells is Z(x) = Z'(x^64), Z'(y) = prod over the missing domain indices i of (y - omega_128^i): one value per cell.
The decoder divides by Z on the coset 7 * domain, where Z takes the value Z'(7^64 * omega_128^brp7(c)) on cell c.

The expected result of a decode is the coefficient list a test started from: nothing here re-implements the decoder."""

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001  # the BLS12-381 scalar field
N_BLOB, N_EXT, N_CELLS, CELL_LEN = 4096, 8192, 128, 64
W8192 = pow(7, (R - 1) // N_EXT, R)  # 7 generates the multiplicative group; the primitive 8192-th root the domains are built from
W128 = pow(W8192, 64, R)
SEVEN64 = pow(7, 64, R)
assert pow(W8192, N_EXT // 2, R) == R - 1 and pow(W128, 64, R) == R - 1


def brp(v, bits):
    r = 0
    for i in range(bits):
        r |= ((v >> i) & 1) << (bits - 1 - i)
    return r


def brp7(c):
    return brp(c, 7)


def fr_be(x):
    return x.to_bytes(32, "big")


def ntt(a, root):
    """[sum_k a[k] root^(i k) for i in range(len(a))] mod R, len(a) a power of two and root a primitive len(a)-th root of unity"""
    n = len(a)
    bits = n.bit_length() - 1
    a = [a[brp(i, bits)] for i in range(n)]
    half = 1
    while half < n:
        step = pow(root, n // (2 * half), R)
        tw = [1] * half
        for j in range(1, half):
            tw[j] = tw[j - 1] * step % R
        for start in range(0, n, 2 * half):
            for j in range(half):
                u, v = a[start + j], a[start + j + half] * tw[j] % R
                a[start + j], a[start + j + half] = (u + v) % R, (u - v) % R
        half *= 2
    return a


def extend(coeffs):
    """the 128 cells (2048 bytes each, as the ABI serialises them) of the polynomial with these coefficients, ascending, at most 8192
    of them (a blob's polynomial has at most 4096: more is an inconsistent codeword)"""
    assert len(coeffs) <= N_EXT
    ev = ntt([c % R for c in coeffs] + [0] * (N_EXT - len(coeffs)), W8192)
    flat = [ev[brp(i, 13)] for i in range(N_EXT)]
    return [b"".join(fr_be(x) for x in flat[CELL_LEN * c:CELL_LEN * (c + 1)]) for c in range(N_CELLS)]


def blob_to_coeffs(evals):
    """the 4096 coefficients of the polynomial whose evaluations, in the blob's (bit-reversed) order, are `evals`"""
    assert len(evals) == N_BLOB
    w4096 = pow(W8192, 2, R)
    nat = [evals[brp(i, 12)] % R for i in range(N_BLOB)]
    inv_n = pow(N_BLOB, R - 2, R)
    return [x * inv_n % R for x in ntt(nat, pow(w4096, R - 2, R))]


def missing_domain_indices(present_cells):
    """domain indices (ascending) of the cells that are NOT in present_cells"""
    have = set(present_cells)
    return sorted(brp7(c) for c in range(N_CELLS) if c not in have)


def cells_of_domain_indices(indices):
    """the cell numbers (ascending) whose domain indices are `indices` (brp7 is its own inverse)"""
    return sorted(brp7(i) for i in indices)


def vanishing(missing):
    """the 65 coefficients, ascending, of prod_{i in missing} (y - omega_128^i); at most 64 roots"""
    assert len(missing) <= 64 and len(set(missing)) == len(missing)
    z = [1]
    for i in missing:
        root = pow(W128, i, R)
        nz = [0] * (len(z) + 1)
        for k, c in enumerate(z):
            nz[k] = (nz[k] - c * root) % R
            nz[k + 1] = (nz[k + 1] + c) % R
        z = nz
    return z + [0] * (65 - len(z))


def poly_eval(z, x):
    acc = 0
    for c in reversed(z):
        acc = (acc * x + c) % R
    return acc


def vanishing_at_cell(z, c):
    """Z'(omega_128^brp7(c)): zero exactly on the missing cells"""
    return poly_eval(z, pow(W128, brp7(c), R))


def vanishing_inverse_on_coset_at_cell(z, c):
    """1 / Z'(7^64 * omega_128^brp7(c)); the coset holds no root of Z'"""
    v = poly_eval(z, SEVEN64 * pow(W128, brp7(c), R) % R)
    assert v != 0
    return pow(v, R - 2, R)
