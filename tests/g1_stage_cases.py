"""Inputs and expected bytes for eth_kzg_amd_test_proofs_from_sums (tests/test_gpu_g1_stage.py, tests/coop_off_check.py): lanes of
known scalars x_j (tests/linmap_model.py plans them) become raw words of the device's signed 13 x 30-bit Jacobian points x_j G, and
the proofs a lane must give are compress(out_k G) with out_k from the map's definition.

The words' digit class is device_ops.JACS -- X: Fs(4, DC), Y and Z: Fs(1, DC) -- which is what the MSM kernels leave in the slots
this hook fills: every form of k_msm_glv.inc ends in to_jacs(acc) (the per-operation test "xyzz_to_jacs" pins that result to
JACS_OUT, the same bounds) or in a fold of such sums by the JacS addition (results JACS_OUT again), stored as they are by
store_sum; an empty MSM leaves the identity of g1_set_inf.  The encoder below covers the class: a fresh random Z per point (equal
points arrive in different representations), coordinates at the ends of their bounds on a share of them, the identity both as
(1 : 1 : 0) and as arbitrary X, Y over Z = 0."""
import random

import numpy as np

import device_ops as D
import linmap_model as M
import oracle_lib

P, R = D.P, M.R
G_BYTES = D.compress(D.G)
IDENTITY = D.compress(None)


def decompress(b):
    """the affine point of a compressed encoding the oracle produced (None: the identity)"""
    if b[0] & 0x40:
        return None
    x = int.from_bytes(b, "big") & ((1 << 381) - 1)
    y = pow((x * x * x + 4) % P, (P + 1) // 4, P)
    assert (y * y - x * x * x - 4) % P == 0
    if bool(b[0] & 0x20) != (y > (P - 1) // 2):
        y = P - y
    return x, y


class Multiples:
    """x -> x G, compressed and affine, from the oracle; every multiple is computed once per process"""

    def __init__(self):
        self.comp, self.aff = {0: IDENTITY}, {0: None}

    def compressed(self, x):
        x %= R
        if x not in self.comp:
            self.comp[x] = oracle_lib.g1_mul(G_BYTES, x.to_bytes(32, "big"))
        return self.comp[x]

    def affine(self, x):
        x %= R
        if x not in self.aff:
            self.aff[x] = decompress(self.compressed(x))
        return self.aff[x]


MULTIPLES = Multiples()
_EXPECTED = {}


def expected_proofs(x, circulant=False):
    """the 128 proofs (48 bytes each, the order the product writes them) of a lane with inputs x, once per distinct vector"""
    key = (tuple(x), circulant)
    if key not in _EXPECTED:
        out = M.proofs_of_circulant_inputs(x) if circulant else M.proofs_of_linmap_inputs(x)
        _EXPECTED[key] = b"".join(MULTIPLES.compressed(v) for v in out)
    return _EXPECTED[key]


def encode(rows, rng):
    """rows[j][lane] = the scalar of the point in slot j of that lane -> int32 words [128][lanes][39]"""
    lanes = len(rows[0])
    out = np.zeros((128, lanes, 39), dtype=np.int64)
    for j in range(128):
        for l in range(lanes):
            a = MULTIPLES.affine(rows[j][l])
            pick = rng.random()
            out[j, l] = D.enc_jacs(a, rng, extreme=pick < 0.25, ident="one" if pick < 0.5 else "junk")
    w = np.ascontiguousarray((out & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
    for pt in w.reshape(-1, 39)[:: max(1, 128 * lanes // 64)]:  # a sample stays inside the class the MSM's sums have
        assert D.JACS.bound_error([int(v) for v in pt]) is None
    return w


def proofs_from_sums(lib, handle, program, n, words):
    """the hook -> (status, [n] byte strings of 128 x 48 bytes)"""
    out = np.zeros((n, 128 * 48), dtype=np.uint8)
    assert words.dtype == np.int32 and words.flags["C_CONTIGUOUS"] and words.shape[0] == 128 and words.shape[2] == 39
    rc = lib.eth_kzg_amd_test_proofs_from_sums(handle, program, n, words.ctypes.data, out.ctypes.data)
    return rc, [out[b].tobytes() for b in range(n)]


def wrong_lanes(got, want):
    """lanes whose proofs differ, with the first differing proof of each"""
    bad = []
    for l, (g, w) in enumerate(zip(got, want)):
        if g != w:
            k = next(k for k in range(128) if g[48 * k:48 * k + 48] != w[48 * k:48 * k + 48])
            bad.append((l, k))
    return bad


_PLANS = {}


def plan(program):
    """(program, degenerate lanes, generic lanes) of tests/linmap_model.py, once per process"""
    if program not in _PLANS:
        p = M.programs()[program]
        pool = M.pool_scalars()
        _PLANS[program] = (p, M.plan_lanes(p, pool), M.generic_lanes(p, pool))
    return _PLANS[program]


def linmap_batches(program, n):
    """the batches of n lanes the plan of `program` runs in -> list of (layout, vectors [n][128])"""
    _, lanes, generic = plan(program)
    return [(b, [M.lane_inputs(e, lanes, generic) for e in b]) for b in M.layout(n, len(lanes))]


def check_linmap_batch(lib, handle, program, run_as, n, batch, vectors, seed):
    """one call of the hook on a planned batch; run_as: the program argument of the hook (-1: the engine's choice).  Asserts every
    lane byte for byte and names the kinds of the wrong lanes."""
    rng = random.Random(seed)
    words = encode([[vectors[l][j] for l in range(n)] for j in range(128)], rng)
    rc, got = proofs_from_sums(lib, handle, run_as, n, words)
    assert rc == 0, rc
    want = [expected_proofs(v) for v in vectors]
    bad = wrong_lanes(got, want)
    assert not bad, (f"program {program} as {run_as}, n = {n}: wrong lanes (lane, kind, first wrong proof): "
                     f"{[(l, batch[l], k) for l, k in bad]}")
