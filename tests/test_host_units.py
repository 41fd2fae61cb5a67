"""Host-side units of the HIP sources that also compile for the CPU (the `HD` functions of csrc/*.hpp): built with
hipcc's host pass and run here, no GPU involved.  The same code runs in the kernels, where tests/test_gpu_parity.py
checks it end to end."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")


def _build_and_run(tmp_path, name, *args):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / name)
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe])
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


@pytest.mark.timeout(600)
def test_binary_gcd_inversion_matches_fermat(tmp_path):
    """csrc/inverse.hpp (used by the Jacobian -> affine step, the host normalisation of the verifier's sums) against a^(p-2): 3000
    draws per field from the whole of [1, m), and 1, 2, m - 2, m - 1, (m +- 1) / 2 and 2^(BITS - 1)."""
    out = _build_and_run(tmp_path, "test_inverse")
    assert out.count(", 0 mismatches") == 2, out


@pytest.mark.timeout(600)
def test_unsaturated_group_law_matches_saturated_formulas(tmp_path):
    """csrc/curve29.hpp + fp29.hpp (14 x 29-bit field, fused a*b + c*d, Z3-based exceptional handling) against the
    plain Jacobian formulas of csrc/curve.hpp: random points, P+P, P-P, identities, mixed chains."""
    out = _build_and_run(tmp_path, "test_curve29")
    assert "0 mismatches" in out


@pytest.mark.timeout(600)
def test_host_multiplication_64_bit_matches_32_bit(tmp_path):
    """csrc/field.hpp: the host's 64-bit-limb Montgomery multiplication against the portable 32-bit CIOS form."""
    out = _build_and_run(tmp_path, "test_host_mul")
    assert "0 mismatches" in out


@pytest.mark.timeout(600)
def test_fk20_proofs_map_compiles_to_its_definition(tmp_path):
    """csrc/g1_linmap.hpp: the two G1 transforms of the prover compiled into a straight-line program of point operations
    (free cyclotomic splits + Karatsuba / Toom-Cook Toeplitz products with the interpolation on the fixed side). Run over
    Fr, the plan and its scheduled slot program must equal IDFT_128 -> keep 64 -> DFT_128; the Hankel building blocks
    are checked for every size and split."""
    out = _build_and_run(tmp_path, "test_linmap")
    assert "0 mismatches" in out and "fk20 plan" in out


@pytest.mark.timeout(600)
def test_unsaturated_fr_matches_saturated_field(tmp_path):
    """csrc/fr29.hpp (9 x 29-bit Fr of the prover's NTT kernels: no carry instructions, Montgomery factor -1) against the
    saturated arithmetic of csrc/field.hpp: products at every bound the kernels use (entry 32 r, 56 r after 12 layers), limb
    re-grouping, the (x << 5) entry from the stored Montgomery form, and the 4096-point Cooley-Tukey network with bit-reversed
    twiddles against the definition of the DFT, without any reduction inside the transform."""
    out = _build_and_run(tmp_path, "test_fr29")
    assert "0 mismatches" in out


@pytest.mark.timeout(600)
def test_glv_split_is_balanced_and_exact(tmp_path):
    """csrc/glv.hpp (the scalar split behind the GLV window table): k1 + k2 lambda == k mod r and |k1|, |k2| <=
    (lambda + 1) / 2 + 1 < 2^127 for 200 k random scalars, small scalars, 0, 1, r - 1, multiples of lambda and the
    branch points of the two balancing steps."""
    out = _build_and_run(tmp_path, "test_glv")
    assert "0 mismatches" in out


@pytest.mark.timeout(600)
def test_host_pairing_building_blocks_and_bilinearity(tmp_path):
    """csrc/host_pairing.cpp: sparse line multiplication, complex and cyclotomic (Granger-Scott) squaring against the
    general Fp12 product on random values; the pairing check on multiples of the trusted setup's [1]_1, [tau]_1 against
    [1]_2, [tau]_2: e(a [tau]_1, [1]_2) e(-a [1]_1, [tau]_2) = 1, the unbalanced pair is not, identities are."""
    out = _build_and_run(tmp_path, "test_pairing", os.path.join(ROOT, "rust-eth-kzg_amd", "data", "trusted_setup_4096.bin"))
    assert "fp12 building blocks: 0 mismatches" in out and "pairing checks: 0 mismatches" in out


@pytest.mark.timeout(900)
def test_signed_13_digit_field_matches_saturated_field_and_python_integers(tmp_path):
    """csrc/fp30.hpp (13 signed 30-bit digits, R = 2^390: the field of the GLV MSM and the constant multiplications) against
    csrc/field.hpp at every operand class (centred, floor digits, lazy differences), the fused product-minus-value forms, the
    one- and two-accumulator product pairs, worst-case digit patterns; then raw digit vectors of 200 rounds against Python's
    integers: out * 2^390 == a * b (mod p), |out| < p, canonical(w) == w mod p."""
    dump = str(tmp_path / "fp30_dump.txt")
    out = _build_and_run(tmp_path, "test_fp30", dump)
    assert "0 mismatches" in out
    p = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
    R = 1 << 390

    def val(d):
        return sum(x << (30 * i) for i, x in enumerate(d))

    rows = [line.split() for line in open(dump)]
    assert len(rows) == 200 * 11
    for i in range(0, len(rows), 11):
        g = {r[0]: val([int(x) for x in r[1:]]) for r in rows[i:i + 11]}
        a, bu, w, cu, du = g["a"], g["bu"], g["w"], g["cu"], g["du"]
        for name, want, bound in (("mulCU", a * bu, 1), ("mulWC_U", w * a, 1), ("sqr", a * a, 1),
                                  ("sqr_inj2", a * a - (cu + 2 * du) * R, 4), ("mul_add_split", a * w + cu * a, 1)):
            assert (g[name] * R - want) % p == 0 and abs(g[name]) < bound * p, name
        assert g["canon_w"] == w % p


@pytest.mark.timeout(900)
def test_signed_13_digit_group_law_matches_saturated_formulas(tmp_path):
    """csrc/curve30.hpp (XYZZ mixed addition with fused subtractions and floor-digit products, the general addition and doubling of
    the folds, exact slow paths, the packed table entry, conversions to and from the 14 x 29-bit form) against csrc/curve.hpp."""
    out = _build_and_run(tmp_path, "test_curve30")
    assert "0 mismatches" in out


# ---- csrc/verify_host.hpp: the host statements the verifiers share, on the CPU against tests/verify_transcript.py -------------------------
def _verify_host_cases():
    """-> [(command line of the case file, expected output line)]: a plain function of the seeds.  The transcripts treat their inputs
    as opaque bytes, so seeded random bytes serve (no curve material)."""
    import hashlib
    import random

    import verify_transcript as T

    rng = random.Random("verify-host:1")
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))  # noqa: E731
    R = T.R
    out = []

    def cell_case(comm, idx):
        cells, proofs = [rb(T.BYTES_PER_CELL) for _ in idx], [rb(48) for _ in idx]
        h = hashlib.sha256()  # the digest next to the challenge: the many path's fold seed hashes it
        uniq, row = T.dedup(comm)
        h.update(b"RCKZGCBATCH__V1_" + T.be64(T.N_BLOB) + T.be64(T.CELL_LEN) + T.be64(len(uniq)) + T.be64(len(idx)) + b"".join(uniq))
        for k in range(len(idx)):
            h.update(T.be64(row[k]) + T.be64(idx[k]) + cells[k] + proofs[k])
        assert T.reduce_digest(h.digest()) == T.cell_challenge(comm, idx, cells, proofs)
        line = "cell %d " % len(idx) + " ".join("%s %d %s %s" % (c.hex(), i, l.hex(), p.hex()) for c, i, l, p in zip(comm, idx, cells, proofs))
        out.append((line, "cell %s %s" % (T.fr_be(T.cell_challenge(comm, idx, cells, proofs)).hex(), h.hexdigest())))
        out.append(("dedup %d " % len(comm) + " ".join(c.hex() for c in comm),
                    "dedup %d %s %s" % (len(uniq), ",".join(map(str, row)), b"".join(uniq).hex())))

    a, b, c = rb(48), rb(48), rb(48)
    cell_case([a], [5])                                   # n = 1
    cell_case([b, b, b], [0, 127, 64])                    # all commitments equal: m = 1
    cell_case([a, b, a, c, b], [9, 9, 10, 127, 0])        # rows 0 1 0 2 1: first-occurrence order, not byte order
    assert T.dedup([a, b, a, c, b])[1] == [0, 1, 0, 2, 1]
    many = [rb(48) for _ in range(7)]
    cell_case([rng.choice(many) for _ in range(130)], list(range(128)) + [3, 3])  # 128 distinct indices plus repeats

    for counts, idx, want in (((3, 3, 3, 3), [0, 64, 127], 0), ((2, 3, 3, 3), [0, 1, 2], 3), ((3, 2, 3, 3), [0, 1], 3), ((3, 3, 2, 3), [0, 1, 2], 3),
                              ((3, 3, 3, 2), [0, 1, 2], 3), ((3, 3, 3, 3), [0, 128, 1], 3), ((0, 0, 0, 0), [], 0), ((1, 1, 1, 1), [1 << 40], 3)):
        out.append(("validate %d %d %d %d %d %s" % (*counts, len(idx), " ".join(map(str, idx))), "validate %d" % want))

    assert 2 * R < 1 << 256 < 3 * R  # so the digests below take the zero-, one- and two-subtraction paths
    for v in (0, R - 1, R, 2 * R - 1, 2 * R, (1 << 256) - 1):
        d = v.to_bytes(32, "big")
        out.append(("reduce " + d.hex(), "reduce " + T.fr_be(T.reduce_digest(d)).hex()))
    out.append(("canonical " + R.to_bytes(32, "big").hex(), "canonical 0 -"))
    out.append(("canonical " + (R - 1).to_bytes(32, "big").hex(), "canonical 1 " + (R - 1).to_bytes(32, "big").hex()))
    out.append(("canonical " + bytes(32).hex(), "canonical 1 " + bytes(32).hex()))

    for _ in range(2):
        blob, comm = rb(131072), rb(48)
        out.append(("blob %s %s" % (blob.hex(), comm.hex()), "blob " + T.fr_be(T.blob_challenge(blob, comm)).hex()))
    for n in (1, 3):
        cs, ps = [rb(48) for _ in range(n)], [rb(48) for _ in range(n)]
        zs, ys = [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]
        zs[0], ys[-1] = R - 1, 0
        line = "blobbatch %d " % n + " ".join("%s %s %s %s" % (c_.hex(), T.fr_be(z).hex(), T.fr_be(y).hex(), p.hex()) for c_, z, y, p in zip(cs, zs, ys, ps))
        out.append((line, "blobbatch " + T.fr_be(T.blob_batch_challenge(cs, zs, ys, ps)).hex()))

    digests = rb(32 * 256)  # the challenges' digests of a pass of 256 problems
    seed = hashlib.sha256(b"RCKZGCBATCHFOLD1" + digests).digest()
    for i in (0, 1, 255):
        w = int.from_bytes(hashlib.sha256(seed + T.be64(i)).digest()[:16], "little") & ((1 << 127) - 1)  # 127 bits of the digest's first 16 bytes
        assert w != 0
        words = [(w >> (32 * j)) & 0xffffffff for j in range(4)]
        assert words[3] >> 31 == 0
        out.append(("fold %s %d" % (digests.hex(), i), "fold %s %s" % (seed.hex(), " ".join("%08x" % x for x in words))))
    out.append(("brp7", "brp7 " + ",".join(str(T.brp(v, 7)) for v in range(128))))
    return out


@pytest.fixture(scope="module")
def verify_host_cases():
    return _verify_host_cases()


# the same stand-alone program twice: as the other host units are built, and with AddressSanitizer + UBSan (its own main, run
# directly: nothing is preloaded and nothing is loaded into Python)
VERIFY_HOST_BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(VERIFY_HOST_BUILDS))
def verify_host_output(request, tmp_path_factory, verify_host_cases):
    """-> {command word: [(expected line, printed line)]} of one build of tests/c/test_verify_host.cpp run over the case file"""
    tmp = tmp_path_factory.mktemp("verify_host_" + request.param)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, cases = str(tmp / "test_verify_host"), str(tmp / "cases.txt")
    subprocess.check_call([hipcc, *VERIFY_HOST_BUILDS[request.param], "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_verify_host.cpp"), "-o", exe])
    with open(cases, "w") as f:
        f.write("".join(line + "\n" for line, _ in verify_host_cases))
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    printed = run.stdout.splitlines()
    assert len(printed) == len(verify_host_cases), run.stdout[-2000:]
    by_command = {}
    for (line, want), got in zip(verify_host_cases, printed):
        by_command.setdefault(line.split()[0], []).append((want, got))
    return by_command


def _same(pairs, count):
    assert len(pairs) == count
    for want, got in pairs:
        assert got == want


@pytest.mark.timeout(600)
def test_cell_batch_transcript_matches_hashlib(verify_host_output):
    """CellBatchTranscript, the ONE statement of the cell verifiers' challenge (single, sharded, device-resident and many paths), and
    dedup_commitments under it: n = 1; three equal commitments; A B A C B (rows and first-occurrence order); 130 cells over all 128
    indices with repeats.  Challenge and raw digest against tests/verify_transcript.py."""
    _same(verify_host_output["cell"], 4)
    _same(verify_host_output["dedup"], 4)


@pytest.mark.timeout(600)
def test_cell_batch_validation_codes(verify_host_output):
    """validate_cell_batch: a valid batch, each of the four length mismatches, an index of 128, an index far beyond 32 bits, n = 0"""
    _same(verify_host_output["validate"], 8)


@pytest.mark.timeout(600)
def test_digest_reduction_and_canonical_scalars(verify_host_output):
    """fr_from_digest on 0, r - 1, r, 2r - 1, 2r, 2^256 - 1 (no, one and two subtractions); fr_from_be_canonical rejects r and accepts
    r - 1 and 0, and fr_to_be gives the bytes back; brp7 on every cell index"""
    _same(verify_host_output["reduce"], 6)
    _same(verify_host_output["canonical"], 3)
    _same(verify_host_output["brp7"], 1)


@pytest.mark.timeout(600)
def test_blob_transcripts_match_hashlib(verify_host_output):
    """blob_challenge on two random 131072-byte blobs (blob_challenge_header is also what the GPU hashes in front of every blob);
    blob_batch_weight for n = 1 and n = 3, z = r - 1 and y = 0 among the values"""
    _same(verify_host_output["blob"], 2)
    _same(verify_host_output["blobbatch"], 2)


@pytest.mark.timeout(600)
def test_fold_weights_match_hashlib(verify_host_output):
    """fold_seed and fold_weight for problems 0, 1 and 255 of a pass of 256: SHA-256(seed | i), its first 16 bytes as four little-endian
    words, 127 bits kept -- the top bit of word 3 is clear"""
    _same(verify_host_output["fold"], 3)
    for _, got in verify_host_output["fold"]:
        assert int(got.split()[-1], 16) >> 31 == 0
