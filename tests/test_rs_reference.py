"""tests/rs_reference.py (the statement tests/test_gpu_rs_decode.py holds the decoder's kernels to) against the CPU oracle and against
itself.  No GPU."""
import random

import pytest

import rs_reference as F

PATTERNS = {
    "even cells": list(range(0, 128, 2)),
    "cells 64-127": list(range(64, 128)),
    "65 random": sorted(random.Random("rs-reference 65").sample(range(128), 65)),
}


@pytest.fixture(scope="module")
def codeword():
    rng = random.Random("rs-reference polynomial")
    coeffs = [rng.randrange(F.R) for _ in range(F.N_BLOB)]
    return coeffs, F.extend(coeffs)


def test_extend_is_the_polynomial_at_the_points_the_cells_stand_for(codeword):
    coeffs, cells = codeword
    assert len(cells) == 128 and all(len(c) == 2048 for c in cells)
    for c, j in [(0, 0), (0, 1), (1, 0), (63, 63), (64, 0), (77, 13), (127, 63)]:  # Horner at h_c * omega_64^brp6(j), one power at a time
        x = pow(F.W8192, F.brp7(c), F.R) * pow(pow(F.W8192, 128, F.R), F.brp(j, 6), F.R) % F.R
        assert cells[c][32 * j:32 * j + 32] == F.fr_be(F.poly_eval(coeffs, x)), (c, j)
    # the blob is cells 0..63, and the inverse transform returns the coefficients
    blob = [int.from_bytes(cells[c][32 * j:32 * j + 32], "big") for c in range(64) for j in range(64)]
    assert F.blob_to_coeffs(blob) == coeffs


@pytest.mark.parametrize("name", list(PATTERNS))
def test_the_oracle_recovers_extends_cells(oracle, codeword, name):
    _, cells = codeword
    present = PATTERNS[name]
    assert len(present) == {"even cells": 64, "cells 64-127": 64, "65 random": 65}[name]
    got, _proofs = oracle.recover_cells_and_kzg_proofs(present, [cells[c] for c in present])
    assert got == cells, name


@pytest.mark.parametrize("name", list(PATTERNS))
def test_vanishing_is_zero_exactly_on_the_missing_cells(name):
    present = PATTERNS[name]
    missing = F.missing_domain_indices(present)
    assert F.cells_of_domain_indices(missing) == [c for c in range(128) if c not in present]
    z = F.vanishing(missing)
    d = len(missing)
    assert len(z) == 65 and z[d] == 1 and not any(z[d + 1:])
    for c in range(128):
        assert (F.vanishing_at_cell(z, c) == 0) == (c not in present), (name, c)
        x = F.SEVEN64 * pow(F.W128, F.brp7(c), F.R) % F.R
        assert F.vanishing_inverse_on_coset_at_cell(z, c) * F.poly_eval(z, x) % F.R == 1


def test_vanishing_of_small_root_sets():
    assert F.vanishing([]) == [1] + [0] * 64
    assert F.vanishing([0]) == [F.R - 1, 1] + [0] * 63  # y - 1
    assert F.vanishing([64]) == [1, 1] + [0] * 63  # omega_128^64 = -1
    assert F.vanishing([0, 64]) == [F.R - 1, 0, 1] + [0] * 62  # y^2 - 1
    z = F.vanishing(list(range(0, 128, 2)))  # the 64 even powers: y^64 - 1
    assert z == [F.R - 1] + [0] * 63 + [1]
    assert F.vanishing(list(range(1, 128, 2))) == [1] + [0] * 63 + [1]  # y^64 + 1
