"""The hook eth_kzg_amd_test_verify_many_sums from Python (tests/test_verify_inputs.py imports many_sums), and, run as a program in a process
of its own with ETH_KZG_AMD_COOP_POINTS=0 (the limit is read once per process) and ETH_KZG_AMD_HOST_THREADS=2: the many-verification
without the four-lane kernels -- k_vm_products<VmLane> with its one-lane subgroup blocks in a short-chain pass, k_vm_fold_mul<VmLane> in a
folded one, from both sources: the expanded problems and the columns of a block (nothing else gives the column source's short-chain
map to the one-lane instantiation) -- compared with the bytes the parent computed with the four-lane kernels on.
stdin: JSON {"seed", "passes": {name: {"sums": [hex or null], "fold": hex or null}},
             "columns": {name: {"picks", "indices", "form": [small, folded], "status", "verified", "sums": [hex], "fold": hex}}}."""
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
kzg = importlib.import_module("rust-eth-kzg_amd")


class ManySums:
    """what one call of the hook handed out"""


def many_sums(ctx, problems, max_probes=256):
    """problems = [(commitments, cell_indices, cells, proofs), ...] -> (return code, ManySums): verified, status, small, folded, searched,
    fold_verdict, sums[B] (96 bytes each), rho[B] (integers), fold (96 bytes), probes [(lo, hi, 96 bytes, passed)], n_probes"""
    lib = kzg.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nb, lens, tabs, _keep = ctx._marshal_many(problems)
    ver, st, form = (C.c_int32 * nb)(), (C.c_int32 * nb)(), (C.c_int32 * 4)()
    sums, rho, fold = C.create_string_buffer(96 * nb), (C.c_uint32 * (4 * nb))(), C.create_string_buffer(96)
    pr, ps, npr = (C.c_int32 * (3 * max_probes))(), C.create_string_buffer(96 * max_probes), C.c_uint64(0)
    rc = lib.eth_kzg_amd_test_verify_many_sums(ctx.handle, nb, vp(lens[0]), vp(tabs[0]), vp(lens[1]), vp(tabs[1]), vp(lens[2]), vp(tabs[2]), vp(lens[3]),
                                               vp(tabs[3]), ver, st, form, sums, rho, fold, pr, ps, max_probes, C.byref(npr))
    out = ManySums()
    out.verified, out.status = [bool(v) for v in ver], list(st)
    out.small, out.folded, out.searched, out.fold_verdict = bool(form[0]), bool(form[1]), bool(form[2]), form[3]
    out.sums = [sums.raw[96 * b:96 * b + 96] for b in range(nb)]
    out.rho = [sum(rho[4 * b + j] << (32 * j) for j in range(4)) for b in range(nb)]
    out.fold, out.n_probes = fold.raw, npr.value
    out.probes = [(pr[3 * q], pr[3 * q + 1], ps.raw[96 * q:96 * q + 96], bool(pr[3 * q + 2])) for q in range(min(npr.value, max_probes))]
    return rc, out


def main():
    import verify_transcript as T
    want = json.load(sys.stdin)
    passes = {p.name: p for p in T.many_cases(want["seed"])}
    ctx = kzg.DASContext(True)
    blobs = T.material_blobs()
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(blobs)
    assert st == [0] * len(blobs)
    comms = [ctx.blob_to_kzg_commitment(b) for b in blobs]
    mat = T.Material(blobs, comms, cells, proofs, [None] * len(blobs))
    for name, exp in want["passes"].items():
        p = passes[name]
        problems = [q.args(mat) for q in p.problems]
        rc, got = many_sums(ctx, problems)
        assert rc == 0, (name, rc)
        assert (got.small, got.folded, got.searched) == (p.small, p.folded, p.searched), (name, got.small, got.folded, got.searched)
        assert got.status == [q.status for q in p.problems] and got.verified == [q.verdict for q in p.problems], (name, got.status, got.verified)
        bad = [b for b, q in enumerate(p.problems) if q.live and got.sums[b].hex() != exp["sums"][b]]
        assert not bad, "%s: problems whose pairing inputs differ from the statement: %s" % (name, bad)
        if p.folded:
            assert got.fold.hex() == exp["fold"] and got.fold_verdict == 1, (name, "the folded pair")
        assert ctx.verify_cell_kzg_proof_batch_many(problems) == (got.verified, got.status), name
    import data_columns as D
    from test_gpu_data_columns import column_sums  # the column tap hook, as that file calls it
    for name, exp in want["columns"].items():
        call = D.block(comms, cells, proofs, exp["picks"], exp["indices"])
        rc, got = column_sums(ctx, call, "host", 0)
        assert rc == 0, (name, rc)
        assert [got.small, got.folded] == exp["form"] and (not got.folded or got.fold_verdict == 1), (name, got.small, got.folded, got.fold_verdict)
        assert (got.status, got.verified) == (exp["status"], exp["verified"]), (name, got.status, got.verified)
        assert [s.hex() for s in got.sums] == exp["sums"] and got.fold.hex() == exp["fold"], (name, "differs from the four-lane kernels")
        rc, same = many_sums(ctx, D.expand(*call))  # column j IS problem j of the expanded input
        assert rc == 0 and (same.small, same.folded, same.status, same.verified) == (got.small, got.folded, got.status, got.verified), name
        assert same.sums == got.sums and same.fold == got.fold, (name, "differs from the expanded pass")
    ctx.close()
    print("many coop-off ok")


if __name__ == "__main__":
    main()
