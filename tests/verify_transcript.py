"""An independent statement of what the batch verifiers pair, and the cases it is compared on (tests/test_verify_inputs.py).

Written from the reference's source, not from oracle/kzg.c and not from csrc/verify_host.hpp or csrc/verify.hip:
  crates/cryptography/kzg_multi_open/src/fk20/verifier.rs:49-65    deduplicate_with_indices (the caller's side: eip7594/src/verifier.rs)
                                                          :129-260  verify_multi_opening: the four lincombs and the two pairing inputs
                                                          :269-384  compute_fiat_shamir_challenge, compute_powers, compute_sum_interpolation_poly
  crates/eip4844/src/verifier.rs:81-143                             verify_blob_kzg_proof_batch: z_i, y_i per blob
                                :201-262                            compute_r_powers_for_verify_kzg_proof_batch
  crates/cryptography/kzg_single_open/src/verifier.rs:59-108        verify_kzg_proof_batch: lhs and rhs

Everything in Fr is hashlib and Python integers.  Only the final sums in G1 go through oracle_lib.g1_msm, which tests/test_verify_msm.py
and tests/test_oracle_units.py pin on their own.  A verdict is one bit that does not depend on the challenge for valid inputs; the 96
bytes of the two pairing inputs depend on every byte of the transcript, every power of r, every weight and every interpolation
coefficient.

The many-verification's fold (its weights, the folded pair, the probes of its search) is stated in its own section below, and
many_cases() holds the passes it is compared on."""
import hashlib
import os
import random

import oracle_lib
import synth

R = synth.R
N_BLOB, CELL_LEN, N_CELLS, BYTES_PER_CELL = 4096, 64, 128, 2048
INF = b"\xc0" + bytes(47)
ONE_BE = (1).to_bytes(32, "big")
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# omega_n = 7^((r - 1) / n): Domain::compute_generator_for_size squares blstrs' ROOT_OF_UNITY = 7^((r - 1) / 2^32) down (polynomial/src/domain.rs:84-101)
W8192 = pow(7, (R - 1) // 8192, R)
W4096 = pow(W8192, 2, R)
W128 = pow(W8192, 64, R)
W64 = pow(W8192, 128, R)
assert pow(W8192, 4096, R) == R - 1 and pow(W64, 32, R) == R - 1


def be64(v):
    return int(v).to_bytes(8, "big")


def fr_be(v):
    return int(v % R).to_bytes(32, "big")


def brp(v, bits):
    return int(format(v, "0%db" % bits)[::-1], 2)


def reduce_digest(d):
    """reduce_bytes_to_scalar_bias (bls12_381/src/lib.rs:128-140): the 256-bit big-endian integer mod r"""
    return int.from_bytes(d, "big") % R


_setup64 = None


def setup_g1_first64():
    """[tau^i]_1, i < 64, compressed: what VerificationKey::commit_g1 commits the interpolation polynomial on (verification_key.rs:66-70)"""
    global _setup64
    if _setup64 is None:
        raw = open(os.path.join(_ROOT, "rust-eth-kzg_amd", "data", "trusted_setup_4096.bin"), "rb").read()
        assert raw[:8] == b"KZGSRS01"
        _setup64 = [raw[16 + 48 * i:16 + 48 * i + 48] for i in range(64)]
    return _setup64


def g1_sum(points):
    """the sum of compressed points (an MSM with every scalar 1)"""
    return oracle_lib.g1_msm(b"".join(points), ONE_BE * len(points))


# ---- the cell verifier ---------------------------------------------------------------------------------------------------------------
def dedup(commitments):
    """deduplicate_with_indices (verifier.rs:49-65): byte equality, first-occurrence order -> (unique commitments, row of every entry)"""
    seen, uniq, row = {}, [], []
    for c in commitments:
        if c not in seen:
            seen[c] = len(uniq)
            uniq.append(c)
        row.append(seen[c])
    return uniq, row


def cell_digest(commitments, indices, cells, proofs):
    """the raw SHA-256 of the cell transcript (verifier.rs:269-328), before it is reduced: 32 bytes"""
    uniq, row = dedup(commitments)
    n = len(indices)
    h = hashlib.sha256()
    h.update(b"RCKZGCBATCH__V1_" + be64(N_BLOB) + be64(CELL_LEN) + be64(len(uniq)) + be64(n))
    h.update(b"".join(uniq))
    for k in range(n):
        h.update(be64(row[k]) + be64(indices[k]))
        h.update(cells[k])
        h.update(proofs[k])
    return h.digest()


def cell_challenge(commitments, indices, cells, proofs):
    """compute_fiat_shamir_challenge (verifier.rs:269-328) -> r.  The transcript covers the whole batch whatever range is evaluated."""
    return reduce_digest(cell_digest(commitments, indices, cells, proofs))


_interp_cache = {}
_W64_INV_POW = [pow(W64, (64 - j) % 64, R) for j in range(64)]  # omega_64^-j


def interp_coeffs(cell, index):
    """The 64 coefficients of the polynomial of degree < 64 that takes the cell's values on its coset (compute_sum_interpolation_poly,
    verifier.rs:348-384, one summand): the cell holds the evaluations bit-reversed; in natural order f(h w^j) = e_j with the coset
    generator h = omega_8192^brp7(index) (cosets.rs:89-112) and w = omega_64, so c_i = h^-i / 64 * sum_j e_j w^(-i j): a plain 64 x 64 sum."""
    key = (cell, index)
    got = _interp_cache.get(key)
    if got is None:
        stored = [int.from_bytes(cell[32 * j:32 * j + 32], "big") for j in range(CELL_LEN)]
        assert all(v < R for v in stored)
        e = [stored[brp(j, 6)] for j in range(CELL_LEN)]
        h_inv = pow(W8192, (8192 - brp(index, 7)) % 8192, R)
        inv64 = pow(64, -1, R)
        got, hi = [], inv64
        for i in range(CELL_LEN):
            s = sum(e[j] * _W64_INV_POW[(i * j) % 64] for j in range(CELL_LEN)) % R
            got.append(s * hi % R)
            hi = hi * h_inv % R
        _interp_cache[key] = got
    return got


def cell_partial_scalars(commitments, indices, cells, proofs, lo, hi, r):
    """-> (uniq, [r^k], [r^k h_k^64], [w_row], [I_i]) for the cells k in [lo, hi): global exponents, weights over the range only"""
    uniq, row = dedup(commitments)
    rk = pow(r, lo, R)
    s1, s2, w, interp, per_cell = [], [], [0] * len(uniq), [0] * CELL_LEN, {}
    for k in range(lo, hi):
        s1.append(rk)
        s2.append(rk * pow(W128, brp(indices[k], 7), R) % R)  # h_c^64 = omega_128^brp7(c): bit_reversed_coset_gens_pow_n
        w[row[k]] = (w[row[k]] + rk) % R
        key = (cells[k], indices[k])  # I = sum_k r^k I_k, with the r^k of a repeated (cell, index) added up first
        per_cell[key] = per_cell.get(key, 0) + rk
        rk = rk * r % R
    for (cell, index), weight in per_cell.items():
        for i, c in enumerate(interp_coeffs(cell, index)):
            interp[i] = (interp[i] + weight * c) % R
    return uniq, s1, s2, w, interp


def cell_partial(commitments, indices, cells, proofs, lo, hi, r=None):
    """The two pairing inputs of the cells [lo, hi) of the batch, compressed: A = sum r^k pi_k, then
    B = sum r^k h_k^64 pi_k + sum w_row C_row - sum I_i [tau^i]_1 as ONE sum over n + m + 64 points (verifier.rs:186-240)."""
    n = len(indices)
    assert len(commitments) == len(cells) == len(proofs) == n and 0 <= lo <= hi <= n
    if r is None:
        r = cell_challenge(commitments, indices, cells, proofs)
    if lo == hi:
        return INF + INF
    uniq, s1, s2, w, interp = cell_partial_scalars(commitments, indices, cells, proofs, lo, hi, r)
    pi = b"".join(proofs[lo:hi])
    a = oracle_lib.g1_msm(pi, b"".join(fr_be(s) for s in s1))
    b = oracle_lib.g1_msm(pi + b"".join(uniq) + b"".join(setup_g1_first64()),
                          b"".join(fr_be(s) for s in s2) + b"".join(fr_be(s) for s in w) + b"".join(fr_be(-s) for s in interp))
    return a + b


# ---- the many-verification's fold ------------------------------------------------------------------------------------------------------
# One pairing check stands for all problems of a pass (csrc/verify_host.hpp: "folding weights of a many-verification pass", DESIGN.md
# section 4, `k_vm_*`): with sum_b = the two pairing inputs of problem b, S_j = sum_b rho_b sum_b[j].  The weights hang on every input byte of the
# pass through the problems' transcript digests.  Written from that definition, not by calling the library.
FOLD_DOMAIN = b"RCKZGCBATCHFOLD1"


def fold_weights(digests, takes_part):
    """digests[i]: the raw 32-byte transcript digest of problem i of the pass (32 zero bytes for a problem that was skipped before it was
    hashed); takes_part[i]: the problem is neither empty nor refused.  seed = SHA-256(domain | all digests in order); rho_i = the first 16
    bytes of SHA-256(seed | be64(i)) as a little-endian integer mod 2^127, 0 -> 1, with i the position in the PASS; rho_i = 0 for a problem
    that takes no part."""
    assert len(digests) == len(takes_part) and all(len(d) == 32 for d in digests)
    seed = hashlib.sha256(FOLD_DOMAIN + b"".join(digests)).digest()
    out = []
    for i, on in enumerate(takes_part):
        v = int.from_bytes(hashlib.sha256(seed + be64(i)).digest()[:16], "little") % (1 << 127)
        out.append((v or 1) if on else 0)
    return out


def fold_pair(sums, rho, lo, hi):
    """compress(S_0) | compress(S_1) over the problems lo <= b < hi: S_j = sum_b rho_b sums[b][j] (sums[b] = the problem's 96 bytes; the
    whole pass is the folded pair, a sub-range is a probe of the search).  Problems of weight 0 take no part, whatever their sums."""
    part = [b for b in range(lo, hi) if rho[b]]
    if not part:
        return INF + INF
    sc = b"".join(fr_be(rho[b]) for b in part)
    return oracle_lib.g1_msm(b"".join(sums[b][:48] for b in part), sc) + oracle_lib.g1_msm(b"".join(sums[b][48:] for b in part), sc)


# ---- the blob batch verifier -----------------------------------------------------------------------------------------------------------
def blob_challenge(blob, commitment):
    """compute_fiat_shamir_challenge (eip4844/src/verifier.rs:155-196): the degree is a 128-bit big-endian integer"""
    return reduce_digest(hashlib.sha256(b"FSBLOBVERIFY_V1_" + (N_BLOB).to_bytes(16, "big") + blob + commitment).digest())


_DOMAIN_BR = None
_eval_cache = {}


def blob_eval(blob, z):
    """y = p(z) for the polynomial whose evaluations on the bit-reversed domain the blob holds (blob_scalar_to_polynomial + eval,
    verifier.rs:118-125), by the barycentric formula p(z) = (z^N - 1) / N * sum_j f_j w_j / (z - w_j) with w_j = omega_4096^brp12(j)"""
    global _DOMAIN_BR
    key = (blob, z)
    if key in _eval_cache:
        return _eval_cache[key]
    if _DOMAIN_BR is None:
        nat = [1] * N_BLOB
        for i in range(1, N_BLOB):
            nat[i] = nat[i - 1] * W4096 % R
        _DOMAIN_BR = [nat[brp(j, 12)] for j in range(N_BLOB)]
    f = [int.from_bytes(blob[32 * j:32 * j + 32], "big") for j in range(N_BLOB)]
    assert all(v < R for v in f)
    if z in _DOMAIN_BR:
        y = f[_DOMAIN_BR.index(z)]
    else:
        # batch inversion of z - w_j
        d = [(z - w) % R for w in _DOMAIN_BR]
        pre, acc = [], 1
        for x in d:
            pre.append(acc)
            acc = acc * x % R
        inv = pow(acc, -1, R)
        s = 0
        for j in range(N_BLOB - 1, -1, -1):
            dj_inv = inv * pre[j] % R
            inv = inv * d[j] % R
            s += f[j] * _DOMAIN_BR[j] % R * dj_inv
        y = (pow(z, N_BLOB, R) - 1) * pow(N_BLOB, -1, R) % R * (s % R) % R
    _eval_cache[key] = y
    return y


def blob_batch_challenge(commitments, zs, ys, proofs):
    """compute_r_powers_for_verify_kzg_proof_batch (verifier.rs:201-262) -> r"""
    n = len(commitments)
    h = hashlib.sha256()
    h.update(b"RCKZGBATCH___V1_" + be64(N_BLOB) + be64(n))
    for c, z, y, p in zip(commitments, zs, ys, proofs):
        h.update(c + fr_be(z) + fr_be(y) + p)
    return reduce_digest(h.digest())


def blob_batch_inputs(blobs, commitments, proofs):
    """-> (r, rhs | lhs compressed): rhs = sum r^i pi_i pairs with [tau]_2, lhs = sum r^i C_i - (sum r^i y_i) G + sum r^i z_i pi_i with
    -[1]_2 (kzg_single_open/src/verifier.rs:76-99)"""
    n = len(blobs)
    assert len(commitments) == len(proofs) == n and n >= 1
    zs = [blob_challenge(b, c) for b, c in zip(blobs, commitments)]
    ys = [blob_eval(b, z) for b, z in zip(blobs, zs)]
    r = blob_batch_challenge(commitments, zs, ys, proofs)
    rp = [pow(r, i, R) for i in range(n)]
    ysum = sum(a * y for a, y in zip(rp, ys)) % R
    gen = setup_g1_first64()[0]
    rhs = oracle_lib.g1_msm(b"".join(proofs), b"".join(fr_be(a) for a in rp))
    lhs = oracle_lib.g1_msm(b"".join(commitments) + gen + b"".join(proofs),
                            b"".join(fr_be(a) for a in rp) + fr_be(-ysum) + b"".join(fr_be(a * z) for a, z in zip(rp, zs)))
    return r, rhs + lhs


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
SEED = "verify-inputs:1"
# blobs of the material: three seeded ones, the zero blob, a constant polynomial, the constant r - 1 (every element the largest canonical one)
B_ZERO, B_CONST, B_MAX = 3, 4, 5
CONST_VALUE = int.from_bytes(hashlib.sha256(b"verify-inputs:constant").digest(), "big") % R


def material_blobs():
    return [synth.seeded_blob(4200 + i) for i in range(3)] + [bytes(131072), fr_be(CONST_VALUE) * N_BLOB, fr_be(R - 1) * N_BLOB]


class Material:
    """blobs (material_blobs()), their commitments, cells[b][128], cell proofs[b][128] and blob proofs, from the library or the oracle"""

    def __init__(self, blobs, commitments, cells, proofs, blob_proofs):
        self.blobs, self.commitments, self.cells, self.proofs, self.blob_proofs = blobs, commitments, cells, proofs, blob_proofs
        # what the special blobs are named for
        assert commitments[B_ZERO] == INF and set(proofs[B_ZERO]) == {INF} and set(cells[B_ZERO]) == {bytes(BYTES_PER_CELL)}
        assert set(cells[B_CONST]) == {fr_be(CONST_VALUE) * CELL_LEN} and set(proofs[B_CONST]) == {INF}
        assert set(cells[B_MAX]) == {fr_be(R - 1) * CELL_LEN} and set(proofs[B_MAX]) == {INF}
        assert len(set(commitments)) == len(commitments)


class CellCase:
    def __init__(self, name, entries, ranges=(), **expect):
        self.name, self.entries, self.expect = name, entries, expect
        n = len(entries)
        self.ranges = [(0, n)] + [rg for rg in ranges if rg != (0, n)]

    def args(self, mat):
        """-> (commitments, indices, cells, proofs): one (blob, cell index) pair per entry; repeated entries share their bytes objects"""
        return ([mat.commitments[b] for b, _ in self.entries], [c for _, c in self.entries],
                [mat.cells[b][c] for b, c in self.entries], [mat.proofs[b][c] for b, c in self.entries])

    def check(self, mat):
        """the case reaches the condition it is named for"""
        comm, idx, _, _ = self.args(mat)
        uniq, row = dedup(comm)
        pop = [row.count(i) for i in range(len(uniq))]
        e = self.expect
        assert len(idx) == e.get("n", len(idx)), self.name
        if "m" in e:
            assert len(uniq) == e["m"], (self.name, len(uniq))
        if "max_row" in e:
            assert max(pop) >= e["max_row"], (self.name, pop)
        if "min_row" in e:
            assert min(pop) == e["min_row"], (self.name, pop)
        if e.get("unsorted"):
            assert uniq != sorted(uniq) and len(uniq) == 4, self.name
            firsts = [row.index(i) for i in range(len(uniq))]
            assert firsts == sorted(firsts) and any(row[k] > row[k + 1] for k in range(len(row) - 1)), self.name  # interleaved
        if e.get("all_indices"):
            assert sorted(set(idx)) == list(range(N_CELLS)), self.name
        if e.get("one_index"):
            assert len(set(idx)) == 1 and len(uniq) > 1, self.name
        if "blobs" in e:
            assert {b for b, _ in self.entries} >= set(e["blobs"]), self.name
        if "only_blobs" in e:
            assert {b for b, _ in self.entries} == set(e["only_blobs"]), self.name
        for lo, hi in self.ranges:
            assert 0 <= lo < hi <= len(idx), (self.name, lo, hi)
        if "bits" in e:  # bits set in the exponents the ranges other than the whole batch evaluate: the table entries r^(2^i) used
            used = 0
            for lo, hi in self.ranges[1:]:
                for k in range(lo, hi):
                    used |= k
            assert used == e["bits"], (self.name, bin(used))
        if "carry" in e:  # a range that crosses a carry into this bit with a non-zero start
            assert any(lo > 0 and (lo >> e["carry"]) != ((hi - 1) >> e["carry"]) for lo, hi in self.ranges[1:]), self.name


LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025)
RANGES_300 = ((0, 1), (299, 300), (5, 200), (255, 257))
N_BIG = 8200
BIG_RANGES = ((8190, 8200), (4090, 4100))


def cell_cases(seed=SEED):
    """every cell-verifier case; a plain function of the seed.  Entries are (blob of the material, cell index)."""
    rng = random.Random(seed)
    rnd = lambda n, blobs=(0, 1, 2): [(rng.choice(blobs), rng.randrange(N_CELLS)) for _ in range(n)]  # noqa: E731
    out = [CellCase("len-%d" % n, rnd(n), n=n) for n in LENGTHS]
    out.append(CellCase("one-commitment", rnd(130, (1,)), m=1, n=130))
    # four commitments, first met in the order 1, 4, 0, 2 (asserted against the byte order in check()), then interleaved
    out.append(CellCase("four-interleaved", [(b, rng.randrange(N_CELLS)) for b in (1, 4, 0, 2)] + rnd(96, (0, 1, 2, 4)), m=4, unsorted=True))
    lone = rnd(19, (2,)) + rnd(280, (0,))
    lone.insert(150, (1, 77))
    out.append(CellCase("row-of-280-next-to-row-of-1", lone, n=300, m=3, max_row=257, min_row=1))
    out.append(CellCase("identity-commitment-only", rnd(66, (B_ZERO,)), m=1, only_blobs=(B_ZERO,)))
    mixed = rnd(40, (0, B_ZERO, 1))
    out.append(CellCase("identity-commitment-mixed", [(B_ZERO, 9)] + mixed, blobs=(0, 1, B_ZERO)))
    out.append(CellCase("one-index", [(b, 101) for b in (0, 1, 2, B_CONST)] + [(rng.choice((0, 1, 2, B_CONST)), 101) for _ in range(126)], one_index=True, m=4))
    every = [(rng.choice((0, 1, 2)), c) for c in range(N_CELLS)]
    rng.shuffle(every)
    out.append(CellCase("all-128-indices", every, all_indices=True, n=128))
    out.append(CellCase("zero-cells", rnd(3, (B_ZERO,)) + rnd(2), blobs=(B_ZERO,)))
    out.append(CellCase("constant-polynomial", rnd(2) + rnd(70, (B_CONST,)) + rnd(1), blobs=(B_CONST,)))
    out.append(CellCase("cells-of-r-minus-1", rnd(1) + rnd(67, (B_MAX,)) + rnd(2, (B_CONST,)), blobs=(B_MAX, B_CONST)))
    out.append(CellCase("ranges-of-300", rnd(300), RANGES_300, n=300))
    # k in [8190, 8200) sets bits 1 .. 13 and, with [4090, 4100), bit 0: table entries 0 .. 13; 4095 -> 4096 carries across bit 12
    out.append(CellCase("exponents-to-2^13", rnd(N_BIG), BIG_RANGES, n=N_BIG, bits=(1 << 14) - 1, carry=12))
    assert len({c.name for c in out}) == len(out)
    return out


# ---- the passes of the many-verification -------------------------------------------------------------------------------------------------
_off_subgroup = None


def off_subgroup_point():
    """a compressed point on the curve and outside the subgroup: the smallest x >= 5 that gives one (the oracle says which)"""
    global _off_subgroup
    x = 5
    while _off_subgroup is None:
        cand = bytearray(x.to_bytes(48, "big"))
        cand[0] |= 0x80
        if oracle_lib.g1_validate(bytes(cand), False) == 0 and oracle_lib.g1_validate(bytes(cand), True) != 0:
            _off_subgroup = bytes(cand)
        x += 1
    return _off_subgroup


class ManyProblem:
    """One problem of a pass: a CellCase as it stands ("valid"), or changed into
      "empty"         no cells: verified without a check, takes no part in the fold (status 0)
      "swapped"       two proofs exchanged (entries `swap`): everything decodes, the sums are exact MSMs, the verdict is False
      "bad-index"     a cell index of 128: refused at validation, before anything is hashed (status 3)
      "bad-scalar"    a cell element r: refused by the decoder (status 1)
      "off-subgroup"  a proof on the curve and outside the subgroup: refused by the subgroup test (status 2)"""
    STATUS = {"valid": 0, "empty": 0, "swapped": 0, "bad-scalar": 1, "off-subgroup": 2, "bad-index": 3}

    def __init__(self, case, kind="valid", swap=None):
        self.case, self.kind, self.swap = case, kind, swap
        self.name = case.name if kind == "valid" else "empty" if kind == "empty" else "%s:%s" % (case.name, kind)
        self.status = self.STATUS[kind]
        self.live = kind in ("valid", "swapped")            # takes part in the sums, the fold and the search
        self.hashed = kind not in ("empty", "bad-index")    # its transcript was hashed (decoding verdicts arrive behind the hashes)
        self.verdict = kind in ("valid", "empty")           # what the public call reports as verified

    def args(self, mat):
        if self.kind == "empty":
            return [], [], [], []
        comm, idx, cells, proofs = (list(col) for col in self.case.args(mat))
        last = len(idx) - 1
        if self.kind == "swapped":
            i, j = self.swap
            assert proofs[i] != proofs[j], self.name
            proofs[i], proofs[j] = proofs[j], proofs[i]
        elif self.kind == "bad-index":
            idx[last] = N_CELLS
        elif self.kind == "bad-scalar":
            cells[last] = cells[last][:-32] + R.to_bytes(32, "big")
        elif self.kind == "off-subgroup":
            proofs[last] = off_subgroup_point()
        return comm, idx, cells, proofs


class ManyPass:
    def __init__(self, name, problems, small, folded, searched=False, **expect):
        self.name, self.problems, self.small, self.folded, self.searched, self.expect = name, problems, small, folded, searched, expect

    def cells(self):
        """n cells and m unique commitments of the pass as the engine counts them: problems refused at validation hold none"""
        n = m = 0
        for q in self.problems:
            if q.kind not in ("empty", "bad-index"):
                n += len(q.case.entries)
                m += len({b for b, _ in q.case.entries})
        return n, m

    def shares(self, i, j):
        """problems i and j both hold cells and carry a commitment in common (entries name blobs; the material's commitments are distinct)"""
        if not (0 <= i < len(self.problems) and 0 <= j < len(self.problems)) or i == j:
            return False
        a, b = self.problems[i], self.problems[j]
        if a.kind in ("empty", "bad-index") or b.kind in ("empty", "bad-index"):
            return False
        return bool({x for x, _ in a.case.entries} & {x for x, _ in b.case.entries})

    def check(self, host_threads, coop_points_max):
        """the pass is one pass, takes the form it is meant to take under `host_threads` helper threads and holds what it is named for
        (the thresholds are csrc/verify_many.hip's expressions)"""
        B = len(self.problems)
        n, m = self.cells()
        live = [q.live for q in self.problems]
        assert n <= 131072 and not (B >= 192 and n >= 24576), self.name                       # neither chunks nor parts
        assert self.small == (B <= 2 * host_threads), (self.name, B)                          # the short-chain form
        assert self.folded == (not self.small and sum(live) >= 2), self.name                  # one folded check
        assert self.searched == (self.folded and not all(q.verdict for q in self.problems if q.live)), self.name
        assert self.problems[0].kind not in ("empty", "bad-index"), self.name                 # problem 0 holds cells: later positions are > 0
        e = self.expect
        if "one_lane" in e:  # k_vm_products<VmQuad> up to 2 * coop_points_max() products and subgroup tests, k_vm_products<VmLane> above
            assert self.small and e["one_lane"] == (3 * n + 2 * m + 64 * B > 2 * coop_points_max), (self.name, n, m, B)
        if "kinds" in e:
            assert sorted(q.kind for q in self.problems) == sorted(e["kinds"]), self.name
        if "wrong" in e:
            assert [i for i, q in enumerate(self.problems) if q.live and not q.verdict] == e["wrong"], self.name
        if "n_problems" in e:
            assert B == e["n_problems"], self.name
        if e.get("sharing_is_adjacent"):  # a problem that shares a commitment with any problem of the pass shares one with a neighbour
            for i in range(B):
                anywhere = any(self.shares(i, j) for j in range(B))
                assert anywhere == (self.shares(i, i - 1) or self.shares(i, i + 1)), (self.name, i)
            assert sum(self.shares(i, i + 1) for i in range(B - 1)) >= e.get("adjacent_pairs", 1), self.name
        if "lonely" in e:  # problems that share no commitment with anyone: they must stay put under a weight that looks next door
            assert [i for i in range(B) if not any(self.shares(i, j) for j in range(B)) and self.problems[i].live] == e["lonely"], self.name
        if "hole_before_live" in e:
            dead = [i for i, q in enumerate(self.problems) if not q.live]
            assert e["hole_before_live"] == bool(dead and any(live[dead[0]:])), self.name


def search_plan(live, verdicts, host_threads):
    """the probes of the search for the wrong problems of a pass, level by level, in the order they are made -- csrc/verify_many.hip's
    expressions: suspects are handed to per-problem checks when they are at most 2 T problems or a quarter of the live ones are suspect
    ranges, else every suspect range is cut K = clamp(T / ranges, 2, 16) ways.  -> [(lo, hi, passes)]"""
    T, B, n_live = host_threads, len(live), sum(live)
    suspects, out = [(0, B)], []
    while suspects:
        if len(suspects) * 4 >= n_live or sum(hi - lo for lo, hi in suspects) <= 2 * T:
            break
        K = min(16, max(2, T // len(suspects)))
        probes = []
        for lo, hi in suspects:
            parts = min(K, hi - lo)
            probes += [(lo + (hi - lo) * q // parts, lo + (hi - lo) * (q + 1) // parts) for q in range(parts)]
        suspects = []
        for lo, hi in probes:
            ok = all(verdicts[b] for b in range(lo, hi) if live[b])
            out.append((lo, hi, ok))
            if not ok and hi - lo > 1:
                suspects.append((lo, hi))
    return out


MANY_HOST_THREADS = 2  # of the context the passes run on: short-chain up to 4 problems, two-way splits, per-problem checks from 4 suspects
SEARCH_WRONG = [0, 150, 299]
SEARCH_EMPTY, SEARCH_REFUSED = 40, 200
LARGE_ORDER = ["len-2", "len-63", "len-1", "len-64", "len-65", "len-255", "len-256", "len-257", "one-commitment", "row-of-280-next-to-row-of-1",
               "all-128-indices", "constant-polynomial", "one-index", "cells-of-r-minus-1", "identity-commitment-only"]

# pass -> kernels of csrc/k_verify_many.hip it reaches (k_vm_scalars, k_vm_weights and k_vm_interp_sum run in every pass)
#   short-four-lanes    k_vm_products<VmQuad> (products, the 64 interpolation terms per problem, subgroup blocks), k_vm_reduce without icommit
#   short-holes         the same with an empty problem, a refused one and zero cells between exact neighbours
#   short-one-lane      k_vm_products<VmLane> (3 n + 2 m + 64 B > 2 coop_points_max()), k_vm_reduce's 128-stride loops, table entries 0 .. 13
#   large-folded        k_vm_products<VmLane>, the commitment window table's MSM, k_vm_reduce, k_vm_fold_mul<VmQuad>, k_vm_fold_sum (B < 128)
#   large-one-live      k_vm_products<VmLane>, k_vm_reduce; no fold below two live problems
#   search              k_vm_fold_sum's stride loop (B > 128), k_vm_fold_ranges at widths above and below 128
#   folded-ten          with the four-lane kernels switched off (a process of its own): k_vm_fold_mul<VmLane>; short-four-lanes there: k_vm_products<VmLane>
#                       and the one-lane subgroup blocks


def many_cases(seed=SEED):
    """every pass of the many-verification; a plain function of the seed.  Problems are the cell cases, or tiny ones of their kind."""
    cc = {c.name: c for c in cell_cases(seed)}
    rng = random.Random(seed + ":many")
    rnd = lambda n, blobs=(0, 1, 2): [(rng.choice(blobs), rng.randrange(N_CELLS)) for _ in range(n)]  # noqa: E731
    V = lambda name: ManyProblem(cc[name])  # noqa: E731
    tiny = lambda name, n: CellCase(name, rnd(n), n=n)  # noqa: E731
    empty = ManyProblem(CellCase("empty", []), "empty")
    out = [ManyPass("short-four-lanes", [V("len-1"), V("len-65"), V("four-interleaved"), V("identity-commitment-mixed")], True, False, one_lane=False),
           ManyPass("short-holes", [V("len-2"), empty, ManyProblem(tiny("five", 5), "off-subgroup"), V("zero-cells")], True, False, one_lane=False,
                    kinds=["valid", "empty", "off-subgroup", "valid"], hole_before_live=True),
           ManyPass("short-one-lane", [V("exponents-to-2^13")], True, False, one_lane=True),
           ManyPass("large-folded", [V(name) for name in LARGE_ORDER], False, True, n_problems=15, sharing_is_adjacent=True, adjacent_pairs=13,
                    lonely=[14], hole_before_live=False),
           ManyPass("large-one-live", [ManyProblem(tiny("three", 3), "bad-scalar"), empty, V("len-63"), ManyProblem(tiny("four", 4), "bad-index"),
                                       ManyProblem(tiny("six", 6), "off-subgroup")], False, False,
                    kinds=["bad-scalar", "empty", "valid", "bad-index", "off-subgroup"])]
    # the search: 300 problems of one to three cells; every problem's first cell is of the blob its predecessor ended on, so that
    # neighbours share commitment bytes; the wrong ones have two different proofs to exchange
    probs, prev = [], rng.choice((0, 1, 2))
    for i in range(300):
        if i == SEARCH_EMPTY:
            probs.append(empty)
            continue
        n = rng.randrange(2, 4) if i in SEARCH_WRONG else rng.randrange(1, 4)
        entries = [(prev, rng.randrange(N_CELLS))] + rnd(n - 1)
        while i in SEARCH_WRONG and entries[0] == entries[-1]:
            entries[-1] = rnd(1)[0]
        prev = entries[-1][0]
        case = CellCase("tiny-%d" % i, entries, n=n)
        probs.append(ManyProblem(case, "swapped", (0, n - 1)) if i in SEARCH_WRONG else ManyProblem(case, "off-subgroup") if i == SEARCH_REFUSED
                     else ManyProblem(case))
    out.append(ManyPass("search", probs, False, True, True, n_problems=300, wrong=SEARCH_WRONG, sharing_is_adjacent=True, adjacent_pairs=290,
                        lonely=[], hole_before_live=True))
    out.append(ManyPass("folded-ten", [V("len-1"), V("len-2"), empty, V("len-63"), V("zero-cells"), V("len-64"), V("identity-commitment-mixed"),
                                       V("len-65"), V("constant-polynomial"), V("four-interleaved")], False, True, n_problems=10,
                        hole_before_live=True))
    assert len({p.name for p in out}) == len(out)
    return out


def table_entries_reached(cases):
    """the entries r^(2^i) of the 24-entry power table (tab[24] in csrc/verify.hip) that some evaluated exponent of the cases uses: the
    bits set in a k of a range (the whole batch included)"""
    used = 0
    for c in cases:
        for lo, hi in c.ranges:
            for k in range(lo, hi):
                used |= k
    return [i for i in range(24) if used >> i & 1]


class BlobCase:
    def __init__(self, name, picks, **expect):
        self.name, self.picks, self.expect = name, picks, expect

    def args(self, mat):
        return [mat.blobs[b] for b in self.picks], [mat.commitments[b] for b in self.picks], [mat.blob_proofs[b] for b in self.picks]

    def check(self, mat):
        e = self.expect
        assert len(self.picks) == e["n"], self.name
        if e.get("zero"):
            i = self.picks.index(B_ZERO)
            assert mat.commitments[B_ZERO] == INF and mat.blob_proofs[B_ZERO] == INF and i >= 0, self.name
        if e.get("repeat"):
            assert len(set(self.picks)) < len(self.picks), self.name


def blob_cases(seed=SEED):
    rng = random.Random(seed + ":blobs")
    many = [0, B_ZERO, 1, 2, B_MAX, B_CONST, 0, 0] + [rng.choice((0, 1, 2, B_ZERO, B_CONST, B_MAX)) for _ in range(9)]
    return [BlobCase("one-blob", [0], n=1), BlobCase("blob-and-zero-blob", [1, B_ZERO], n=2, zero=True),
            BlobCase("repeated-triple", [2, B_MAX, 2], n=3, repeat=True), BlobCase("seventeen", many, n=17, zero=True, repeat=True)]
