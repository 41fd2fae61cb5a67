"""Caller-supplied trusted setups on the GPU (eth_kzg_amd_das_context_new_with_setup): the mainnet points through the new door
against the golden vectors, an insecure setup with a known secret against the CPU oracle on the same bytes and against closed
forms that use no KZG code, two setups alive on one GPU (the table registry must key on the setup), the wide tables, and every
rejection.  Contexts use small tables (use_precomp=False: 2.4 GB, or a 3 GB budget) so that two setups fit side by side."""
import importlib
import os
import subprocess
import sys
import threading

import pytest

import oracle_lib
import setup_material as sm
import synth
import vectors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
kzg = importlib.import_module("rust-eth-kzg_amd")
R = sm.R


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    # the torch wheel carries its own HIP runtime: it must have been initialised before the engine's (system) runtime, or it finds
    # no GPU -- same order as tests/test_gpu_parity.py
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def custom_points(tmp_path_factory):
    return sm.insecure_setup(tmp_path_factory.getbasetemp())


@pytest.fixture(scope="module")
def custom_oracle(custom_points):
    o = sm.SetupOracle(*custom_points, use_precomp=True, threads=min(8, os.cpu_count() or 1))
    yield o
    o.close()


@pytest.fixture(scope="module")
def custom_ctx(custom_points):
    c = kzg.DASContext.from_trusted_setup(*custom_points, check_powers=True, use_precomp=False)
    yield c
    c.close()


def sparse_blob():
    b = bytearray(kzg.BYTES_PER_BLOB)
    for i, v in ((0, 1), (77, R - 1), (4095, 0x1234567)):
        b[32 * i:32 * i + 32] = v.to_bytes(32, "big")
    return bytes(b)


ZERO_BLOB = bytes(kzg.BYTES_PER_BLOB)


def _norm(x):
    return [_norm(y) for y in x] if isinstance(x, (list, tuple)) else x


# ---- 1. mainnet through the new door -----------------------------------------------------------------------------------------
def test_mainnet_points_reproduce_the_golden_vectors_and_share_the_default_tables():
    g1, g2 = sm.mainnet_points()
    default = kzg.DASContext(use_precomp=False)
    one = default.table_bytes()
    c = kzg.DASContext.from_trusted_setup(g1, g2, check_powers=True, use_precomp=False)
    try:
        assert c.setup_digest == default.setup_digest == sm.digest(g1, g2)
        assert c.table_bytes() == one == default.table_bytes()
        import torch
        free_two = torch.cuda.mem_get_info()[0]
        n = 0
        families = (("blob_to_kzg_commitment", lambda i: c.blob_to_kzg_commitment(i["blob"])),
                    ("compute_cells_and_kzg_proofs", lambda i: c.compute_cells_and_kzg_proofs(i["blob"])),
                    ("verify_cell_kzg_proof_batch", lambda i: c.verify_cell_kzg_proof_batch(i["commitments"], i["cell_indices"], i["cells"], i["proofs"])),
                    ("recover_cells_and_kzg_proofs", lambda i: c.recover_cells_and_kzg_proofs(i["cell_indices"], i["cells"])),
                    ("compute_kzg_proof", lambda i: c.compute_kzg_proof(i["blob"], i["z"])),
                    ("compute_blob_kzg_proof", lambda i: c.compute_blob_kzg_proof(i["blob"], i["commitment"])),
                    ("verify_kzg_proof", lambda i: c.verify_kzg_proof(i["commitment"], i["z"], i["y"], i["proof"])),
                    ("verify_blob_kzg_proof", lambda i: c.verify_blob_kzg_proof(i["blob"], i["commitment"], i["proof"])),
                    ("verify_blob_kzg_proof_batch", lambda i: c.verify_blob_kzg_proof_batch(i["blobs"], i["commitments"], i["proofs"])))
        for fam, call in families:
            for name, case in sorted(vectors.load(fam).items()):
                try:
                    got = call(case["input"])
                except kzg.KzgError:
                    got = None  # the vectors record an Err as null
                assert _norm(got) == _norm(case["output"]), (fam, name)
                n += 1
        assert n == 311, n
        # a second context on the same digest costs no second set of tables
        assert abs(free_two - torch.cuda.mem_get_info()[0]) < 1.0e9
    finally:
        c.close()
        default.close()


# ---- 2. a custom setup against the oracle on the same bytes -----------------------------------------------------------------------
def test_custom_setup_matches_the_oracle_on_every_operation(custom_ctx, custom_oracle, custom_points):
    c, o = custom_ctx, custom_oracle
    assert c.setup_digest == sm.digest(*custom_points)
    blobs = [synth.seeded_blob(900 + i) for i in range(3)] + [sparse_blob(), ZERO_BLOB]
    comms = [c.blob_to_kzg_commitment(b) for b in blobs]
    assert comms == [o.blob_to_kzg_commitment(b) for b in blobs]
    assert comms[-1] == bytes([0xc0]) + bytes(47)
    expect = {}

    def want(blob):
        if blob not in expect:
            expect[blob] = o.compute_cells_and_kzg_proofs(blob)
        return expect[blob]

    for n in (1, 3, 64, 300):  # circulant, cooperative and large-batch schedules
        batch = [blobs[i % len(blobs)] for i in range(n)]
        status, cells, proofs = c.compute_cells_and_kzg_proofs_batch(batch)
        assert status == [0] * n
        for i in range(n):
            ec, ep = want(batch[i])
            assert cells[i] == ec and proofs[i] == ep, (n, i)
    cells, proofs = want(blobs[0])
    keep = list(range(0, 128, 2))
    assert _norm(c.recover_cells_and_kzg_proofs(keep, [cells[k] for k in keep])) == [cells, proofs]
    z = (0x1234567890abcdef << 64 | 5).to_bytes(32, "big")
    for b in (blobs[0], blobs[3], ZERO_BLOB):
        assert tuple(c.compute_kzg_proof(b, z)) == tuple(o.compute_kzg_proof(b, z))
    bp = [c.compute_blob_kzg_proof(b, cm) for b, cm in zip(blobs, comms)]
    assert bp == [o.compute_blob_kzg_proof(b, cm) for b, cm in zip(blobs, comms)]
    # verifiers: true on these outputs, false after one proof is swapped
    idx = [0, 5, 127, 64]
    cm4, ce4, pr4 = [comms[0]] * 4, [cells[k] for k in idx], [proofs[k] for k in idx]
    assert c.verify_cell_kzg_proof_batch(cm4, idx, ce4, pr4) is True
    swapped = [pr4[1], pr4[0]] + pr4[2:]
    assert c.verify_cell_kzg_proof_batch(cm4, idx, ce4, swapped) is False
    c2, p2 = want(blobs[1])
    problems = [(cm4, idx, ce4, pr4), ([comms[1]] * 2, [3, 9], [c2[3], c2[9]], [p2[3], p2[9]]), (cm4, idx, ce4, swapped)]
    verdicts, status = c.verify_cell_kzg_proof_batch_many(problems)
    assert verdicts == [True, True, False] and status == [0, 0, 0]
    pz, y = c.compute_kzg_proof(blobs[0], z)
    pz2, _ = c.compute_kzg_proof(blobs[1], z)
    assert c.verify_kzg_proof(comms[0], z, y, pz) is True and c.verify_kzg_proof(comms[0], z, y, pz2) is False
    assert c.verify_blob_kzg_proof(blobs[0], comms[0], bp[0]) is True and c.verify_blob_kzg_proof(blobs[0], comms[0], bp[1]) is False
    assert c.verify_blob_kzg_proof_batch(blobs[:3], comms[:3], bp[:3]) is True
    assert c.verify_blob_kzg_proof_batch(blobs[:3], comms[:3], [bp[1], bp[0], bp[2]]) is False


# ---- 3. closed forms on the known secret: no KZG code on the reference side ---------------------------------------------------
def test_commitment_and_proofs_equal_the_closed_form_on_the_known_secret(custom_ctx, custom_points):
    gen = custom_points[0][:48]

    def times_g(k):
        k %= R
        return oracle_lib.g1_mul(gen, k.to_bytes(32, "big")) if k else bytes([0xc0]) + bytes(47)

    for seed in (910, 911):
        blob = synth.seeded_blob(seed)
        p_tau = sm.eval_blob_at(blob, sm.TAU)
        assert custom_ctx.blob_to_kzg_commitment(blob) == times_g(p_tau)
        cells, proofs = custom_ctx.compute_cells_and_kzg_proofs(blob)
        for k in (0, 37, 127):
            i_tau, h64 = sm.cell_interpolant_at(cells[k], k, sm.TAU)
            q = (p_tau - i_tau) * pow(pow(sm.TAU, 64, R) - h64, R - 2, R)
            assert proofs[k] == times_g(q), (seed, k)


# ---- 4. two setups alive at once on one GPU -----------------------------------------------------------------------------------
def test_two_setups_on_one_gpu_keep_their_own_tables(custom_points, custom_oracle, oracle):
    """The window-table registry keys on the setup's digest: without it the second context picks up the first one's tables and
    returns well-formed proofs of the wrong setup."""
    blobs = [synth.seeded_blob(920 + i) for i in range(4)]
    want_main = [oracle.compute_cells_and_kzg_proofs(b) for b in blobs]
    want_cust = [custom_oracle.compute_cells_and_kzg_proofs(b) for b in blobs]
    assert want_main[0][1] != want_cust[0][1]

    def check_pair(main, cust):
        assert main.setup_digest != cust.setup_digest
        errors = []

        def run(ctx, want, orc):
            try:
                for rnd in range(3):
                    for b, (ec, ep) in zip(blobs, want):
                        cells, proofs = ctx.compute_cells_and_kzg_proofs(b)
                        assert cells == ec and proofs == ep, "prover bytes differ from this setup's oracle"
                        cm = ctx.blob_to_kzg_commitment(b)
                        assert cm == orc.blob_to_kzg_commitment(b)
                        assert ctx.verify_cell_kzg_proof_batch([cm] * 3, [1, 2, 100], [ec[1], ec[2], ec[100]], [ep[1], ep[2], ep[100]]) is True
            except Exception as e:  # noqa: BLE001
                errors.append(repr(e))

        th = [threading.Thread(target=run, args=(main, want_main, oracle)), threading.Thread(target=run, args=(cust, want_cust, custom_oracle))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
        # proofs made under one setup do not verify under the other
        (ec, ep), b = want_main[0], blobs[0]
        cm_main, cm_cust = main.blob_to_kzg_commitment(b), cust.blob_to_kzg_commitment(b)
        assert cust.verify_cell_kzg_proof_batch([cm_main] * 2, [4, 9], [ec[4], ec[9]], [ep[4], ep[9]]) is False
        assert main.verify_cell_kzg_proof_batch([cm_cust] * 2, [4, 9], [ec[4], ec[9]], [want_cust[0][1][4], want_cust[0][1][9]]) is False

    for order in ("main first", "custom first"):
        main = kzg.DASContext(use_precomp=False)
        cust = kzg.DASContext.from_trusted_setup(*custom_points, use_precomp=False)
        try:
            assert main.table_bytes() == cust.table_bytes() > 0
            check_pair(main, cust)
        finally:
            for c in ((main, cust) if order == "main first" else (cust, main)):
                c.close()
    again = kzg.DASContext.from_trusted_setup(*custom_points, use_precomp=True, table_budget_gb=3)
    try:
        for b, (ec, ep) in zip(blobs, want_cust):
            assert tuple(again.compute_cells_and_kzg_proofs(b)) == (ec, ep)
    finally:
        again.close()


# ---- 5. wide tables from the supplied bases -----------------------------------------------------------------------------------
def test_wide_tables_are_built_from_the_supplied_bases(custom_points, custom_oracle):
    saved = os.environ.pop("ETH_KZG_AMD_TABLE_GB", None)  # the library's default budget
    try:
        c = kzg.DASContext.from_trusted_setup(*custom_points, use_precomp=True, wait_tables=False)
        try:
            first = c.compute_cells_and_kzg_proofs(synth.seeded_blob(930))  # on the start tables, while the wide ones are built
            assert tuple(first) == custom_oracle.compute_cells_and_kzg_proofs(synth.seeded_blob(930))
            assert c.tables_ready(-1) == 1
            assert (c.window_bits(), c.window_count()) == (15, 9), "the default budget gives the nine-window tables"
            blobs = [synth.seeded_blob(930 + i % 7) for i in range(64)]
            status, cells, proofs = c.compute_cells_and_kzg_proofs_batch(blobs)
            assert status == [0] * 64
            for i in range(7):
                ec, ep = custom_oracle.compute_cells_and_kzg_proofs(blobs[i])
                for j in range(i, 64, 7):
                    assert cells[j] == ec and proofs[j] == ep, j
            assert c.blob_to_kzg_commitment(blobs[1]) == custom_oracle.blob_to_kzg_commitment(blobs[1])
        finally:
            c.close()
    finally:
        if saved is not None:
            os.environ["ETH_KZG_AMD_TABLE_GB"] = saved


# ---- 6. rejections ------------------------------------------------------------------------------------------------------------
def _swap(points, size, i, new):
    return points[:size * i] + new + points[size * (i + 1):]


def test_bad_setups_are_rejected_without_abort_or_leak(custom_points, tmp_path):
    """Every case is NULL + Err (a KzgError here) with the promised message; in a child process, so that an abort fails this test and
    not the run; device memory before and after the rejections is compared as the constructor-fault test does."""
    g1, g2 = custom_points
    other_g2 = sm.g2_powers(sm.TAU_OTHER)
    tau1_g1, tau1_g2 = g1[:48] * sm.N_G1, g2[:96] * sm.N_G2
    off1 = sm.g1_off_subgroup_point()
    assert oracle_lib.g1_validate(off1, False) == 0 and oracle_lib.g1_validate(off1, True) != 0
    off2 = sm.g2_compress(sm.g2_off_subgroup_point())
    inf1 = bytes([0xc0]) + bytes(47)
    mat = tmp_path / "material"
    mat.mkdir()
    # g1_monomial[513] plus a point of order 11 (tests/small_order.py): what an attacker sends, where off1 is a hash-made curve point
    import small_order
    st, p513 = small_order.decode(g1[48 * 513:48 * 514])
    assert st == 0
    plus11 = small_order.encode(small_order.d.g_add(p513, small_order.small_order_points()[11]))
    assert oracle_lib.g1_validate(plus11, False) == 0 and oracle_lib.g1_validate(plus11, True) != 0
    files = {"g1": g1, "g2": g2, "other_g2": other_g2, "tau1_g1": tau1_g1, "tau1_g2": tau1_g2, "off1": off1, "off2": off2, "inf1": inf1,
             "plus11": plus11}
    for k, v in files.items():
        (mat / k).write_bytes(v)
    code = (
        "import importlib, os, re, sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch; torch.cuda.init()\n"
        "import setup_material as sm\n"
        "kzg = importlib.import_module('rust-eth-kzg_amd')\n"
        "M = {k: open(os.path.join(%r, k), 'rb').read() for k in %r}\n"
        "g1, g2 = M['g1'], M['g2']\n"
        "sw = lambda pts, size, i, new: pts[:size * i] + new + pts[size * (i + 1):]\n"
        "def rejected(pattern, a, b, **kw):\n"
        "    try:\n"
        "        kzg.DASContext.from_trusted_setup(a, b, use_precomp=False, **kw)\n"
        "    except kzg.KzgError as e:\n"
        "        assert str(e).startswith('ContextCreation(') and re.search(pattern, str(e)), (pattern, str(e))\n"
        "        return\n"
        "    raise SystemExit('accepted: ' + pattern)\n"
        "def good(**kw):\n"
        "    kzg.DASContext.from_trusted_setup(g1, g2, use_precomp=False, **kw).close()\n"
        "def all_rejections():\n"
        "    for i in (0, 2077, 4095):\n"
        "        rejected(r'g1_monomial\\[%%d\\] is not in the prime-order subgroup' %% i, sw(g1, 48, i, M['off1']), g2)\n"
        "    rejected(r'g1_monomial\\[1\\] is not in the prime-order subgroup', sw(g1, 48, 1, M['off1']), g2)\n"
        "    rejected(r'g1_monomial\\[513\\] is not in the prime-order subgroup', sw(g1, 48, 513, M['plus11']), g2)\n"
        "    rejected(r'g1_monomial\\[9\\] is not the encoding', sw(g1, 48, 9, bytes([g1[48 * 9] & 0x7f]) + g1[48 * 9 + 1:48 * 10]), g2)\n"
        "    rejected(r'g1_monomial\\[9\\] is not the encoding', sw(g1, 48, 9, bytes([0xe0]) + bytes(47)), g2)\n"
        "    rejected(r'g1_monomial\\[300\\] is the point at infinity', sw(g1, 48, 300, M['inf1']), g2)\n"
        "    rejected(r'g1_monomial\\[300\\] is the point at infinity', sw(g1, 48, 300, M['inf1']), g2, subgroup_check=False)\n"
        "    rejected(r'g2_monomial\\[64\\] is not in the prime-order subgroup', g1, sw(g2, 96, 64, M['off2']))\n"
        "    swapped = sw(sw(g1, 48, 7, g1[48 * 8:48 * 9]), 48, 8, g1[48 * 7:48 * 8])\n"
        "    rejected(r'g1_monomial is not a sequence of consecutive powers', swapped, g2, check_powers=True)\n"
        "    rejected(r'not a sequence of consecutive powers', g1, M['other_g2'], check_powers=True)\n"
        "    rejected(r'degenerate trusted setup', M['tau1_g1'], M['tau1_g2'])\n"
        "    rejected(r'degenerate trusted setup', M['tau1_g1'], M['tau1_g2'], check_powers=True)\n"
        "free = lambda: torch.cuda.mem_get_info()[0]\n"
        "good(check_powers=True); all_rejections()   # warm: what the HIP runtime keeps per process is in\n"
        "m0 = free()\n"
        "for k in range(4): good()\n"
        "m1 = free()\n"
        "all_rejections()\n"
        "m2 = free()\n"
        "print('GROWTH four good cycles %%.2f GB, one round of rejections %%.2f GB' %% ((m0 - m1) / 1e9, (m1 - m2) / 1e9))\n"
        "assert (m1 - m2) <= max(m0 - m1, 0) + 0.3e9, 'rejected setups keep device memory'\n"
        "# the honest file and mainnet pass the structure check; swapped entries load when nobody asks for it\n"
        "good(check_powers=True)\n"
        "kzg.DASContext.from_trusted_setup(*sm.mainnet_points(), use_precomp=False, check_powers=True).close()\n"
        "# from_json_unchecked: a point off the subgroup loads (not at index 1, which calibrates the endomorphism)\n"
        "c = kzg.DASContext.from_trusted_setup(sw(g1, 48, 2077, M['off1']), g2, use_precomp=False, subgroup_check=False)\n"
        "assert c.blob_to_kzg_commitment(bytes(kzg.BYTES_PER_BLOB)) == bytes([0xc0]) + bytes(47)\n"
        "c.close()\n"
        "print('REJECTIONS OK')\n" % (ROOT, os.path.join(ROOT, "tests"), str(mat), sorted(files)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "REJECTIONS OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
