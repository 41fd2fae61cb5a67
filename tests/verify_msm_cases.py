"""Cases, item lists and exact references for the verifier's two-job bucket MSM on its own (csrc/k_verify.hip through
eth_kzg_amd_test_verify_msm; tests/test_verify_msm.py).

A verification feeds this MSM Fiat-Shamir output on seeded random proofs, which never gives a bucket method what makes it go wrong: one
affine point many times in a bucket (the P + P branch of the mixed addition, equal partial sums in the folds), P and -P in a bucket (the
identity in the middle of a sum), inputs related by the structure the method itself adds -- 2^(8p) P and phi(P) = lambda P of OTHER inputs
are then the same affine point --, scalars whose GLV halves are all one byte, and counts so small that most slices of the counting sort
are empty.  Every point here is a known multiple of the generator, so which items share a bucket, which of them are the same affine
point and which buckets sum to the identity is exact integer arithmetic on discrete logarithms, no group operation needed.

Run as a program (by the test, with ETH_KZG_AMD_COOP_POINTS=0: the limit is read once per process) it sends every case through one form
and writes the compressed sums and the status words as JSON."""
import ctypes as C
import functools
import random

import device_ops as D

R = D.R_ORDER
LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF  # eigenvalue of phi(x, y) = (beta x, y) on G1 (csrc/glv.hpp)
assert LAMBDA * LAMBDA + LAMBDA + 1 == R

# 129 crosses the 128 lanes of a bucket's block, 200 x 32 items fill buckets past one round of lanes, 66 = 1 + 1 + 64 is a one-cell verification
COUNTS = [(1, 1), (1, 66), (3, 68), (31, 32), (63, 64), (64, 129), (129, 200)]
POOL_SIZE = 200


def split(k):
    """k = k1 + k2 lambda, k1 = k mod lambda: the unsigned split of glv_split_unsigned"""
    return k % LAMBDA, k // LAMBDA


def join(k1, k2):
    k = k1 + k2 * LAMBDA
    assert k1 < LAMBDA and k < R and split(k) == (k1, k2)
    return k


def rep(byte, n=16):
    return int.from_bytes(bytes([byte]) * n, "big")


# both halves with every byte equal: all 32 items of a point in one bucket.  A half is < lambda + 2 and lambda's top byte is 0xac, so
# 16 equal bytes go up to 0xab; the all-255 half has 15 bytes (its 16th item falls into bucket 0, which is never summed)
S01, S80, SAB = join(rep(0x01), rep(0x01)), join(rep(0x80), rep(0x80)), join(rep(0xAB), rep(0xAB))
SFF = join(rep(0xFF, 15), rep(0xFF, 15))
EDGE = [0, 1, 2, 255, 256, LAMBDA - 1, LAMBDA, LAMBDA + 1, 2 * LAMBDA, R - 1, 2 ** 128 - 1]


class Case:
    """points: discrete logarithms to the generator (None: the identity); job 0 = sum_{i < n0} sc0[i] P_i, job 1 the same with sc1 / n1"""

    def __init__(self, name, dlogs, sc0, sc1):
        self.name, self.dlogs, self.sc = name, [None if d is None else d % R for d in dlogs], (list(sc0), list(sc1))
        self.n = (len(sc0), len(sc1))
        assert (self.n[0], self.n[1]) in COUNTS and len(dlogs) == self.n[1], name
        assert all(0 <= k < R for s in self.sc for k in s) and all(d != 0 for d in self.dlogs), name

    def points(self):
        return [point_of(d) for d in self.dlogs]

    def point_bytes(self):
        return b"".join(D.compress(a) for a in self.points())

    def scalar_bytes(self, job):
        return b"".join(k.to_bytes(32, "big") for k in self.sc[job])

    def nontrivial_terms(self, job):
        return sum(1 for k, d in zip(self.sc[job], self.dlogs) if k and d is not None)

    def expected_dlog(self, job):
        """the sum as a multiple of the generator: the third, group-free opinion"""
        return sum(k * d for k, d in zip(self.sc[job], self.dlogs) if d is not None) % R

    # ---- what the kernels build: the items of every bucket -------------------------------------------------------------------------
    def shifted_buckets(self, job):
        """byte-shifted form: ONE window; bucket b holds, for every scalar i and byte position p, the copy 2^(8p) P_i if byte p of k1 is
        b, and phi(2^(8p) P_i) if byte p of k2 is b.  -> {b: [(i, phi, p, dlog of that copy or None)]}"""
        out = {}
        for i, (k, d) in enumerate(zip(self.sc[job], self.dlogs)):
            for phi, half in enumerate(split(k)):
                for p in range(16):
                    b = (half >> (8 * p)) & 255
                    out.setdefault(b, []).append((i, phi, p, None if d is None else d * pow(2, 8 * p, R) * pow(LAMBDA, phi, R) % R))
        return out

    def windowed_buckets(self, job):
        """windowed form: sixteen 8-bit windows over the pairs (P_i, k1), (phi P_i, k2) -> {(w, b): [(i, phi, dlog or None)]}"""
        out = {}
        for i, (k, d) in enumerate(zip(self.sc[job], self.dlogs)):
            for phi, half in enumerate(split(k)):
                for w in range(16):
                    out.setdefault((w, (half >> (8 * w)) & 255), []).append((i, phi, None if d is None else d * pow(LAMBDA, phi, R) % R))
        return out

    def empty_hist_slices(self, job):
        """k_ps_hist / k_ps_scatter cut the E = 2n half-scalar entries into 64 slices [E s / 64, E (s + 1) / 64)"""
        E = 2 * self.n[job]
        return sum(1 for s in range(64) if E * s // 64 == E * (s + 1) // 64)


@functools.lru_cache(maxsize=None)
def point_of(d):
    return None if d is None else D.g_mul(D.G, d)


@functools.lru_cache(maxsize=None)
def pool():
    """the discrete logarithms of the random points every case draws from"""
    rng = random.Random("verify-msm:pool")
    return [rng.randrange(1, R) for _ in range(POOL_SIZE)]


def _rand_scalars(rng, n):
    return [rng.randrange(1, R) for _ in range(n)]


def _cycle(xs, n, start=0):
    return [xs[(start + i) % len(xs)] for i in range(n)]


def cases(seed=1):
    """Every case of the module as a plain function of the seed."""
    pl = pool()
    out = []

    def add(name, dlogs, sc0, sc1):
        out.append(Case(name, dlogs, sc0, sc1))

    def rng_of(name):
        return random.Random("verify-msm:%d:%s" % (seed, name))

    # 1. baseline: random points, random scalars, every pair of counts
    for n0, n1 in COUNTS:
        name = "baseline-%d-%d" % (n0, n1)
        rng = rng_of(name)
        add(name, pl[:n1], _rand_scalars(rng, n0), _rand_scalars(rng, n1))
    # 2. one point in every slot: random scalars, then scalars whose halves are one byte repeated
    for n0, n1 in ((1, 1), (129, 200)):
        name = "one-point-random-scalars-%d-%d" % (n0, n1)
        rng = rng_of(name)
        add(name, [pl[3]] * n1, _rand_scalars(rng, n0), _rand_scalars(rng, n1))
    for tag, k, (n0, n1) in (("01", S01, (64, 129)), ("80", S80, (129, 200)), ("ab", SAB, (64, 129)), ("ff", SFF, (129, 200))):
        add("one-point-halves-%s-%d-%d" % (tag, n0, n1), [pl[4]] * n1, [k] * n0, [k] * n1)
    add("one-point-halves-mixed-129-200", [pl[5]] * 200, _cycle([S01, SFF, S80, SAB], 129), _cycle([SAB, S80, S01, SFF], 200, 1))
    # 3. P, -P, P, -P, ... with equal scalars: an even count sums to the identity, an odd count to the extra term
    for tag, k, (n0, n1) in (("random", None, (63, 64)), ("halves-80", S80, (64, 129)), ("halves-01", S01, (129, 200)), ("one", 1, (3, 68))):
        name = "plus-minus-%s-%d-%d" % (tag, n0, n1)
        k = rng_of(name).randrange(1, R) if k is None else k
        add(name, [pl[6] if i % 2 == 0 else -pl[6] for i in range(n1)], [k] * n0, [k] * n1)
    # 4. inputs related by what the method adds: byte-shifted copies and phi images of P as inputs of their own
    d = pl[7]
    related = [d, d << 8, d << 64, d << 120, d * LAMBDA, d * LAMBDA << 8, -d * LAMBDA]
    for n0, n1 in ((3, 68), (31, 32)):
        # every half the byte 7: all copies of all seven inputs meet in bucket 7
        add("related-halves-07-%d-%d" % (n0, n1), related + pl[10:10 + n1 - 7], [join(rep(7), rep(7))] * n0, [join(rep(7), rep(7))] * n1)
        # random scalars with planted bytes: byte 1 of k1[0] = byte 0 of k1[1] (2^8 P twice), byte 8 of k1[0] = byte 0 of k1[2] (2^64 P), byte 15
        # of k1[0] = byte 0 of k1[3], byte 0 of k2[0] = byte 0 of k1[4] = byte 0 of k1[6] (lambda P, lambda P and -lambda P), byte 1 of
        # k2[0] = byte 0 of k1[5]
        name = "related-planted-%d-%d" % (n0, n1)
        rng = rng_of(name)
        scs = []
        for n in (n0, n1):
            s = _rand_scalars(rng, n)
            k1, k2 = split(s[0])
            k1 = k1 & ~(0xFF << 8) & ~(0xFF << 64) & ~(0xFF << 120) | (0x31 << 8) | (0x32 << 64) | (0x33 << 120)
            k2 = k2 & ~0xFFFF | 0x3534
            s[0] = join(k1, k2)
            for i, b in ((1, 0x31), (2, 0x32), (3, 0x33), (4, 0x34), (5, 0x35), (6, 0x34)):
                if i < n:
                    a1, a2 = split(s[i])
                    s[i] = join(a1 & ~0xFF | b, a2)
            scs.append(s)
        add(name, related + pl[10:10 + n1 - 7], scs[0], scs[1])
    # 5. edge scalars on distinct random points; then every scalar 0
    for n0, n1 in ((3, 68), (31, 32)):
        add("edge-scalars-%d-%d" % (n0, n1), pl[20:20 + n1], _cycle(EDGE, n0, 5), _cycle(EDGE, n1))
    for n0, n1 in ((1, 1), (63, 64)):
        add("zero-scalars-%d-%d" % (n0, n1), pl[30:30 + n1], [0] * n0, [0] * n1)
    # 6. the identity as an input: here and there, everywhere, in the first and in the last lane (the one the padding lanes repeat)
    name = "identity-some-64-129"
    rng = rng_of(name)
    where = set(rng.sample(range(129), 40))
    add(name, [None if i in where else pl[i] for i in range(129)], _rand_scalars(rng, 64), _rand_scalars(rng, 129))
    name = "identity-everywhere-31-32"
    rng = rng_of(name)
    add(name, [None] * 32, _rand_scalars(rng, 31), _rand_scalars(rng, 32))
    for n0, n1 in ((1, 66), (129, 200)):
        name = "identity-first-and-last-%d-%d" % (n0, n1)
        rng = rng_of(name)
        add(name, [None] + pl[1:n1 - 1] + [None], _rand_scalars(rng, n0), _rand_scalars(rng, n1))
    # 7. the jobs share the point array, the strides of the halves and n_max: one structured, the other random
    name = "asymmetric-structured-job0-64-129"
    rng = rng_of(name)
    add(name, [pl[8]] * 64 + pl[64:129], [S01] * 64, _rand_scalars(rng, 129))
    name = "asymmetric-structured-job1-64-129"
    rng = rng_of(name)
    add(name, [pl[9]] * 129, _rand_scalars(rng, 64), [SAB] * 129)
    assert len({c.name for c in out}) == len(out)
    return out


def case_names():
    return [c.name for c in all_cases()]


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(cases())


def case(name):
    return next(c for c in all_cases() if c.name == name)


# ---- references ---------------------------------------------------------------------------------------------------------------------
def group_law_msm(points, scalars):
    """sum k_i P_i with the affine group law of device_ops.py alone: one doubling per bit, one addition per set bit"""
    acc = None
    for bit in range(max([k.bit_length() for k in scalars] + [1]) - 1, -1, -1):
        acc = D.g_add(acc, acc)
        for a, k in zip(points, scalars):
            if (k >> bit) & 1:
                acc = D.g_add(acc, a)
    return acc


@functools.lru_cache(maxsize=None)
def reference_group_law(name):
    c = case(name)
    pts = c.points()
    return tuple(D.compress(group_law_msm(pts[:c.n[j]], c.sc[j])) for j in (0, 1))


@functools.lru_cache(maxsize=None)
def reference_oracle(name):
    import oracle_lib
    c = case(name)
    pb = c.point_bytes()
    return tuple(oracle_lib.g1_msm(pb[:48 * c.n[j]], c.scalar_bytes(j)) for j in (0, 1))


def reference(name):
    """the group law where a case has few non-trivial terms, the oracle's MSM otherwise (test_verify_msm.py holds the two against
    each other on every case, without a GPU)"""
    c = case(name)
    return reference_group_law(name) if max(c.nontrivial_terms(0), c.nontrivial_terms(1)) <= 48 else reference_oracle(name)


# ---- the hook -----------------------------------------------------------------------------------------------------------------------
def run_form(lib, handle, c, form):
    """-> (sum of job 0, sum of job 1, status words) of eth_kzg_amd_test_verify_msm"""
    out = C.create_string_buffer(96)
    st = (C.c_int32 * c.n[1])(*([-1] * c.n[1]))
    rc = lib.eth_kzg_amd_test_verify_msm(handle, form, c.point_bytes(), c.n[1], c.scalar_bytes(0), c.n[0], c.scalar_bytes(1), c.n[1], out, st)
    assert rc == 0, "%s: eth_kzg_amd_test_verify_msm(form %d) returned %d" % (c.name, form, rc)
    return out.raw[:48], out.raw[48:], list(st)


def main(argv):
    import importlib
    import json
    import os
    import sys
    form, path = int(argv[1]), argv[2]
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    kzg = importlib.import_module("rust-eth-kzg_amd")
    lib = kzg.load_library()
    ctx = kzg.DASContext(use_precomp=True)
    res = {}
    for c in all_cases():
        a, b, st = run_form(lib, ctx.handle, c, form)
        res[c.name] = [a.hex(), b.hex(), st]
    ctx.close()
    with open(path, "w") as f:
        json.dump(res, f)
    print("verify-msm child ok")


if __name__ == "__main__":
    import sys
    main(sys.argv)
