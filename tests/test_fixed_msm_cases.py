"""What tests/test_gpu_fixed_msm.py relies on, checked without a GPU: the schedule model reaches every committed event of
tests/golden/fixed_msm_events.json, the planned halves are what the device's split returns, and the closed forms -- the colliding
setup's bases, the commitment table's layout, commitments and proofs for a known secret -- agree with the CPU oracle."""
import random

import pytest

import device_ops as D
import fixed_msm_cases as F
import oracle_lib
import setup_material as sm
import synth

R = F.R


@pytest.mark.parametrize("width", F.WIDTHS)
def test_every_committed_event_is_reached_by_its_case(width):
    cs = {c.name: c for c in F.cases(width)}
    rows = [r for r in F.required_events() if r[0] == width]
    assert len(rows) > 50 and {r[1] for r in rows} == set(F.KERNELS)
    seen = {}
    for _, kernel, event, place, name in rows:
        if (kernel, name) not in seen:
            seen[(kernel, name)] = {(e, p) for e, p, _ in F.model(cs[name], width, kernel)[0]}
        assert (event, place) in seen[(kernel, name)], (width, kernel, event, place, name)
    # what the issue of this stage names, by place: both degenerate paths in every chain position, in every fold and in the last addition
    have = {(k, e, p) for _, k, e, p, _ in rows}
    W = D.glv_windows(width)
    for ev in ("equal", "opposite"):
        for k in ("chunked", "windowed1", "windowed2"):
            assert {(k, ev, "chain first"), (k, ev, "chain last")} <= have, (k, ev)
            assert (k, "acc identity", "chain restart") in have
        assert (("chunked", "equal", "chain") in have) and (("windowed1", "equal", "chain") in have)  # behind a non-trivial prefix
        assert {("chunked", ev, "fold k1"), ("chunked", ev, "fold k2"), ("chunked", ev, "fold phi")} <= have
        for k in ("windowed1", "windowed2"):
            assert {(k, ev, "tree span 1"), (k, ev, "tree span 2"), (k, ev, "tree span 4")} <= have, (k, ev)
        if W & (W - 1) == 0:  # the k1 sum against phi(k2 sum) is one addition of the tree
            assert ("windowed1", ev, "tree span %d" % W) in have and ("windowed2", ev, "tree span %d" % W) in have
        else:  # nine windows: the pairs mix the halves; the tree's last addition instead
            assert ("windowed1", ev, "tree span 16") in have
        for k in ("flat256", "flat128"):
            assert (k, ev, "fold span 32") in have
    assert len(F.unreachable()) == 5


@pytest.mark.parametrize("width", F.WIDTHS)
def test_nothing_stated_unreachable_is_reached(width):
    """The flat kernel's chains are plain (model() asserts it for every case it replays), its first fold level never doubles or
    cancels, and the collision of bases 31 and 32 is none for two lanes per window."""
    cs = F.cases(width)
    for kernel in ("flat256", "flat128"):
        got = F.reached(width, kernel, cs)
        assert not [k for k in got if k[1].startswith("chain")]
        assert ("equal", "fold phi") not in got and ("opposite", "fold phi") not in got
    assert ("equal", "fold span 64") not in F.reached(width, "flat256", cs) and ("opposite", "fold span 64") not in F.reached(width, "flat256", cs)
    straddle, W = next(c for c in cs if c.name == "bases 31 and 32"), D.glv_windows(width)  # (nine windows: lanes 0 and 18 meet where sums 0-15 take 16-31)
    assert ("equal", "chain first") in {(e, p) for e, p, _ in F.model(straddle, width, "windowed1")[0]}
    two = F.model(straddle, width, "windowed2")[0]
    assert not [e for e, p, _ in two if p.startswith("chain")] and [p for e, p, _ in two if e == "equal"] == ["tree span %d" % (2 * W if W & (W - 1) == 0 else 16)]


@pytest.mark.parametrize("width", F.WIDTHS)
def test_planned_halves_are_what_the_split_returns(width):
    for c in F.cases(width):
        assert all(abs(h) < 1 << 127 for pair in c.halves for h in pair)
        if c.minus_zero:
            assert c.presplit()[15] == 0x80 and c.presplit()[31] == 0x80 and c.presplit()[:15] == bytes(15)
            continue
        assert c.round_trips(), c.name
        assert len(c.canonical()) == len(c.presplit()) == 64 * 32
        assert sum(int.from_bytes(c.canonical()[32 * i:32 * i + 32], "big") for i in range(64)) % R == c.total()


def test_split_statement_on_the_edges_of_its_cells():
    lam = F.LAMBDA
    for k in [0, 1, R - 1, lam, lam - 1, lam + 1, (lam - 1) // 2, (lam + 1) // 2, (lam + 1) // 2 + 1, lam * ((lam + 1) // 2) % R, R - lam, ((lam + 1) // 2 + 1) * lam % R]:
        k1, k2 = F.split_balanced(k)
        assert F.join(k1, k2) == k and abs(k1) <= (lam + 1) // 2 + 1 and abs(k2) <= (lam + 1) // 2 + 1, hex(k)


def test_bases_of_the_colliding_setup_match_the_oracles_transform():
    vec = F.G_BYTES * 63 + F.IDENTITY * 65
    out = oracle_lib.g1_fft(vec, inverse=False)
    for j in (0, 1, 64, 127):
        assert F.c_fk20(j) != 0
        assert out[48 * j:48 * j + 48] == F.times_g(F.c_fk20(j)), j
    assert all(F.c_fk20(j) for j in range(128))
    assert F.c_fk20(0) == 63


def test_expected_sum_agrees_with_the_exact_group_law_on_a_sample():
    rng = random.Random(5)
    few = F.Case("sample", F._rand_halves(rng, 6))
    assert F.expected(0, 5, few.total()) == F.group_law_sum(0, 5, few.halves)
    assert F.expected(1, 5, few.total()) == F.group_law_sum(1, 5, few.halves)


def test_commitment_table_layout_folds_to_the_commitment(oracle):
    """Coefficient k is scalar (group k // 64, base k % 64) of the commitment's MSM launch and the table's bases are the setup's points
    in that order: the 64 group sums of a sparse polynomial, by the oracle's MSM on the mainnet points, add up to its commitment."""
    g1 = sm.mainnet_points()[0]
    rng = random.Random(9)
    coeffs = [0] * 4096
    for k in (0, 63, 64, 65, 2077, 4095):
        coeffs[k] = rng.randrange(R)
    assert [F.commitment_layout(k) for k in (0, 63, 64, 4095)] == [(0, 0), (0, 63), (1, 0), (63, 63)]
    acc = None
    for g in range(64):
        ks = [k for k in range(4096) if coeffs[k] and F.commitment_layout(k)[0] == g]
        if ks:
            pts = b"".join(g1[48 * (64 * g + F.commitment_layout(k)[1]):][:48] for k in ks)
            acc = D.g_add(acc, _decompress(oracle_lib.g1_msm(pts, b"".join(coeffs[k].to_bytes(32, "big") for k in ks))))
    assert D.compress(acc) == oracle.blob_to_kzg_commitment(F.blob_of_coefficients(coeffs))


def _decompress(b):
    if b[0] & 0x40:
        return None
    x = int.from_bytes(bytes([b[0] & 0x1F]) + b[1:], "big")
    y = pow((x ** 3 + 4) % D.P, (D.P + 1) // 4, D.P)
    if (y > (D.P - 1) // 2) != bool(b[0] & 0x20):
        y = D.P - y
    return x, y


def test_closed_forms_for_a_known_secret_match_the_oracle(tmp_path_factory):
    """commitment = p(tau) G and proof_k = q_k(tau) G with q_k by exact polynomial division, against the CPU oracle on the insecure
    setup of tests/setup_material.py; the GPU test uses the same code at tau = 1."""
    pts = sm.insecure_setup(tmp_path_factory.getbasetemp())
    o = sm.SetupOracle(*pts)
    try:
        blob = synth.seeded_blob(941)
        coeffs = F.blob_coefficients(blob)
        assert F.blob_of_coefficients(coeffs) == blob
        assert F.commitment_scalar(coeffs, sm.TAU) == sm.eval_blob_at(blob, sm.TAU)
        assert o.blob_to_kzg_commitment(blob) == F.times_g(F.commitment_scalar(coeffs, sm.TAU))
        cells, proofs = o.compute_cells_and_kzg_proofs(blob)
        for k in (0, 37, 127):
            assert proofs[k] == F.times_g(F.proof_scalar(coeffs, k, sm.TAU)), k
    finally:
        o.close()
    # tau = 1: the commitment's scalar is the blob's element 0, and cell 0 (h^64 = 1) has a proof all the same
    assert F.commitment_scalar(coeffs, 1) == int.from_bytes(blob[:32], "big")
    assert F.proof_scalar(coeffs, 0, 1) == sum(sum(coeffs[64 * m + i] for i in range(64)) * (m) for m in range(64)) % R


def test_the_oracle_computes_on_the_colliding_setup_and_agrees_with_the_closed_forms():
    o = sm.SetupOracle(*F.colliding_setup())
    try:
        coeffs = [1] * 4096
        blob = F.blob_of_coefficients(coeffs)
        assert o.blob_to_kzg_commitment(blob) == F.times_g(4096) == F.times_g(F.commitment_scalar(coeffs, 1))
        proofs = o.compute_cells_and_kzg_proofs(blob)[1]
        for k in (0, 1, 127):
            assert proofs[k] == F.times_g(F.proof_scalar(coeffs, k, 1)), k
    finally:
        o.close()
