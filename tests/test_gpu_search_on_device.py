"""The search of the "many" verifications for their wrong entries with its pairings on the GPU (csrc/vm_search.hpp, k_pairing_check),
through the public calls: eth_kzg_amd_verify_kzg_proof_many, eth_kzg_amd_verify_blob_kzg_proof_many and
eth_kzg_amd_verify_cell_kzg_proof_batch_many, host form and device form each.

ETH_KZG_AMD_GPU_PAIRING_MIN is read once per context, so there are two contexts: one made with =1 (every batch of probes goes to the GPU)
and one with =0 (none does).  200 point items, 24 blob items, 130 one-cell problems plus four 8-cell problems; 0 wrong, one wrong, about
30 % wrong and all wrong, with entries refused at validation or at decoding in between.  Wrongness is planted as the tests of the three
calls plant it (a changed y or another item's proof; another blob's proof; another cell's proof).
  - `verified` and `status` equal the construction under both values, and are identical under both;
  - the tapped probe lists (lo, hi, passed) are identical under both;
  - the search-stats hook reports probes checked on the device under =1 whenever there was a search, and none under =0.
The hooks and DeviceItems / DeviceArrays helpers are the ones of the three calls' own tests."""
import ctypes as C
import importlib
import os

import pytest

import blob_many as BM
import many_leaf as M  # noqa: F401  (DeviceArrays flattens with it)
import point_many as PM
import synth
import test_gpu_blob_many as TB
import test_gpu_many_leaf as TL
import test_gpu_point_many as TP

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu
R = synth.R
PATTERNS = ["none", "one", "third", "all"]


def _ctx(**env):
    import torch
    torch.cuda.init()
    env = dict(env, ETH_KZG_AMD_TABLE_GB="3")  # the start tables: results never depend on the table
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return kzg.DASContext(use_precomp=True)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    """(the context whose search runs on the GPU, the one whose search runs on the host threads)"""
    on, off = _ctx(ETH_KZG_AMD_GPU_PAIRING_MIN="1"), _ctx(ETH_KZG_AMD_GPU_PAIRING_MIN="0")
    yield on, off
    on.close()
    off.close()


def stats(ctx):
    out = (C.c_uint64 * 4)()
    assert kzg.load_library().eth_kzg_amd_test_search_stats(ctx.handle, out) == 0
    return out[0], out[1]


def wrong_places(pattern, n, refused):
    """the entries that get a wrong proof (the refused ones keep their place and stay refused)"""
    live = [i for i in range(n) if i not in refused]
    return {"none": [], "one": live[len(live) * 2 // 5:][:1], "third": [i for i in live if i * 7 % 10 < 3], "all": live}[pattern]


# ---- material: made once, shared by the cases, never changed ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def point_pool(ctxs):
    ctx = ctxs[1]
    zs = synth.seeded_scalars(2, b"search-on-device:z")
    good = []
    for b in range(3):
        blob = synth.seeded_blob(60 + b)
        comm = ctx.blob_to_kzg_commitment(blob)
        for zb in zs:
            proof, y = ctx.compute_kzg_proof(blob, zb)
            good.append((comm, zb, y, proof))
    assert len(set(good)) == 6
    return good


@pytest.fixture(scope="module")
def blob_pool(oracle):
    good = []
    for b in range(4):
        blob = synth.seeded_blob(70 + b)
        comm = oracle.blob_to_kzg_commitment(blob)
        good.append((blob, comm, oracle.compute_blob_kzg_proof(blob, comm)))
    return good


@pytest.fixture(scope="module")
def cell_material(ctxs):
    blobs = [synth.seeded_blob(80), synth.seeded_blob(81)]
    st, cells, proofs = ctxs[1].compute_cells_and_kzg_proofs_batch(blobs)
    assert st == [0, 0]
    return [ctxs[1].blob_to_kzg_commitment(b) for b in blobs], cells, proofs


def point_case(pool, pattern):
    n, refused = 200, {50: "z=r", 150: "bad-commitment-and-z=r"}
    wrong = wrong_places(pattern, n, refused)
    items, ver, st = [], [], []
    for i in range(n):
        c, z, y, p = pool[i % 6]
        if i in refused:
            item, status = PM.error_order_items(pool[i % 6])[refused[i]]
            items.append(item), ver.append(False), st.append(status)
        elif i in wrong:  # a changed y, or the next item's proof
            items.append((c, z, PM.fr_be((int.from_bytes(y, "big") + 1) % R), p) if i % 2 else (c, z, y, pool[(i + 1) % 6][3]))
            ver.append(False), st.append(0)
        else:
            items.append(pool[i % 6]), ver.append(True), st.append(0)
    return items, ver, st


def blob_case(pool, pattern):
    n, refused = 24, {5, 17}
    wrong = wrong_places(pattern, n, refused)
    items, ver, st = [], [], []
    for i in range(n):
        blob, comm, proof = pool[i % 4]
        if i in refused:  # an element of the blob is r itself
            items.append((BM.with_element(blob, 9, R), comm, proof)), ver.append(False), st.append(1)
        elif i in wrong:
            items.append((blob, comm, pool[(i + 1) % 4][2])), ver.append(False), st.append(0)
        else:
            items.append(pool[i % 4]), ver.append(True), st.append(0)
    return items, ver, st


def cell_case(material, pattern):
    comms, cells, proofs = material
    shapes = [1] * 65 + [8, 8] + [1] * 65 + [8, 8]  # 130 one-cell problems and four 8-cell problems
    n, refused = len(shapes), {40: "index", 100: "point"}
    assert n == 134 and shapes.count(1) == 130
    wrong = wrong_places(pattern, n, refused)
    problems, ver, st = [], [], []
    for b, size in enumerate(shapes):
        blob, first = b % 2, (b * 5) % 120
        idx = list(range(first, first + size))
        pr = [proofs[blob][k] for k in idx]
        status = 0
        if b in wrong:
            pr[-1] = proofs[blob][(idx[-1] + 1) % 128]  # the next cell's proof
            assert pr[-1] != proofs[blob][idx[-1]]
        if refused.get(b) == "index":
            idx, status = [128], 3  # refused at validation, before anything is staged
        elif refused.get(b) == "point":
            pr, status = [PM.off_subgroup_point()], 2  # refused at decoding
        problems.append(([comms[blob]] * size, idx, [cells[blob][k] for k in range(first, first + size)], pr))
        ver.append(status == 0 and b not in wrong), st.append(status)
    return problems, ver, st


# ---- the three calls -----------------------------------------------------------------------------------------------------------------------
def run_points(ctx, items, where):
    ver, st = TP.run(ctx, items, where)
    rc, got = TP.sums(ctx, items, where)
    assert rc == 0 and (got.verified, got.status) == (ver, st)
    return ver, st, [(p[0], p[1], p[2], p[3]) for p in got.probes], got.n_probes


def run_blobs(ctx, items, where):
    ver, st = TB.run(ctx, items, where)
    rc, got = TB.sums(ctx, items, where)
    assert rc == 0 and (got.verified, got.status) == (ver, st)
    return ver, st, [(p[0], p[1], p[2], p[3]) for p in got.probes], got.n_probes


def run_cells(ctx, problems, where):
    leaf = where == "device"  # the device form with leaf-hashed challenges (nothing comes down to be hashed), the host form with the reference's
    if where == "host":
        ver, st = ctx.verify_cell_kzg_proof_batch_many(problems)
    else:
        ver, st = TL.DeviceArrays(problems).call(ctx, leaf)
    rc, got = TL.many_sums(ctx, problems, where, TL.LEAF if leaf else 0, max_probes=1024)
    assert rc == 0 and (got.verified, got.status) == (ver, st)
    return ver, st, [(p[0], p[1], p[3]) for p in got.probes], got.n_probes


def both_routes(ctxs, run, entries, want_ver, want_st, where):
    on, off = ctxs
    ver1, st1, probes1, n1 = run(on, entries, where)
    dev1, listed1 = stats(on)
    ver0, st0, probes0, n0 = run(off, entries, where)
    dev0, listed0 = stats(off)
    print("probes", n1, n0, "on the device", dev1, dev0, "wrong", want_ver.count(False))
    assert (ver1, st1) == (want_ver, want_st)
    assert (ver0, st0) == (want_ver, want_st)
    assert n1 == n0 == len(probes1) and probes1 == probes0  # the same probes in the same order with the same outcome
    assert (listed1, listed0) == (n1, n0)
    searched = any(s == 0 and not v for v, s in zip(want_ver, want_st))
    assert dev0 == 0
    assert dev1 > 0 if searched else dev1 == 0
    assert dev1 >= n1 or not searched  # under = 1 every probe of the list ran there (the cell form's last stage besides)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_verify_kzg_proof_many(ctxs, point_pool, pattern, where):
    both_routes(ctxs, run_points, *point_case(point_pool, pattern), where)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_verify_blob_kzg_proof_many(ctxs, blob_pool, pattern, where):
    both_routes(ctxs, run_blobs, *blob_case(blob_pool, pattern), where)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_verify_cell_kzg_proof_batch_many(ctxs, cell_material, pattern, where):
    both_routes(ctxs, run_cells, *cell_case(cell_material, pattern), where)
