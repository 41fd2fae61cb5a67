"""The many-verification: the parent commit's call, this build's unflagged call, and the flagged and device-resident forms, one process, one GPU.

    python tools/time_verify_many_leaf.py --parent-lib PATH [--shapes 1024x128,64x128,8x8192] [--rounds 25]
                                          [--out profiles/verify_many_leaf.json]
    ETH_KZG_AMD_TRACE=1 python tools/time_verify_many_leaf.py --laps [--shapes 1024x128]

Shapes are PROBLEMS x CELLS: problem b holds CELLS cells of 64 distinct blobs (CELLS / 64 of each, at least the 128 cells of blob b mod 64
when CELLS = 128), all valid.  Per shape, on default tables, after three warm-up calls of every kind, --rounds interleaved rounds; a
round times every kind once, the order rotating from round to round; host clock around each call (all are synchronous: they return
verdicts).  Kinds:
    parent_many        eth_kzg_amd_verify_cell_kzg_proof_batch_many of --parent-lib (a libc_eth_kzg.so built from the parent commit, loaded
                       next to this build's, with a context of its own): the baseline
    many               the same symbol of this build
    many_ex_leaf       eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex with ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT, pointer tables marshalled once
    device_leaf        eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex with the flag, flat arrays resident in HBM
    device_reference   the same with flags = 0 (the reference's challenges: proofs and cells come down; the slow way)
Reported per kind: median, minimum, 10th and 90th percentile in milliseconds.  Every timed call must verify every problem.  Two
conditions are evaluated and written next to the figures: `many` within the parent's own p10 .. p90 spread of the parent's median (read
as: the two medians no further apart than the parent's p90 - p10; whether the median lies inside the parent's interval can be read off
the recorded percentiles), and whether device_leaf is faster than parent_many.  --laps: no timing; with ETH_KZG_AMD_TRACE=1 in the environment the library prints the
laps of one call of each of many / many_ex_leaf / device_leaf / device_reference per shape on stderr, behind a line that names the call."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_BLOBS = 64
KINDS = ["parent_many", "many", "many_ex_leaf", "device_leaf", "device_reference"]


def random_blobs(n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, 4096, 32), dtype=np.uint8)
    a[:, :, 0] &= 0x3F  # < 2^254 < r: canonical field elements
    return a.reshape(n, 131072)


def summary(ms):
    s = sorted(ms)
    pick = lambda q: s[min(len(s) - 1, int(q * len(s)))]  # noqa: E731
    return {"median_ms": statistics.median(s), "min_ms": s[0], "p10_ms": pick(0.10), "p90_ms": pick(0.90), "calls": len(s)}


class ParentLibrary:
    """the parent commit's product library, loaded next to this build's: its own context, its eth_kzg_amd_verify_cell_kzg_proof_batch_many"""

    def __init__(self, path, kzg):
        self.lib = C.CDLL(os.path.abspath(path))
        P, U64 = C.c_void_p, C.c_uint64
        self.lib.eth_kzg_amd_das_context_new_on_device.restype = P
        self.lib.eth_kzg_amd_das_context_new_on_device.argtypes = [C.c_bool, C.c_int]
        self.lib.eth_kzg_amd_tables_ready.argtypes = [P, C.c_int]
        self.lib.eth_kzg_das_context_free.argtypes = [P]
        self.lib.eth_kzg_free_error_message.argtypes = [P]
        fn = self.lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many
        fn.restype = kzg.CResult
        fn.argtypes = [P, U64, P, P, P, P, P, P, P, P, P, P]
        assert os.path.realpath(path) != os.path.realpath(kzg.load_library()._name), "--parent-lib is the library under test itself"
        self.ctx = C.c_void_p(self.lib.eth_kzg_amd_das_context_new_on_device(True, 0))
        while self.lib.eth_kzg_amd_tables_ready(self.ctx, 1000) == 0:
            pass

    def many(self, nb, lens, tabs, ver, st):
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        res = self.lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many(self.ctx, nb, vp(lens[0]), vp(tabs[0]), vp(lens[1]), vp(tabs[1]), vp(lens[2]),
                                                                    vp(tabs[2]), vp(lens[3]), vp(tabs[3]), ver, st)
        assert res.status == 0, C.string_at(res.error_msg)

    def close(self):
        self.lib.eth_kzg_das_context_free(self.ctx)


def shape_problems(n_problems, n_cells, comms, cells, proofs):
    """-> problems as (commitments, indices, cells, proofs): n_cells / 64 cells of each of the 64 blobs (n_cells = 128: the 128 cells of one)"""
    out = []
    for b in range(n_problems):
        if n_cells == 128:
            blobs = [(b % N_BLOBS, c) for c in range(128)]
        else:
            per = n_cells // N_BLOBS
            blobs = [(j, (b * per + c) % 128) for j in range(N_BLOBS) for c in range(per)]
        out.append(([comms[j] for j, _ in blobs], [c for _, c in blobs], [cells[j][c] for j, c in blobs], [proofs[j][c] for j, c in blobs]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x128,64x128,8x8192")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--laps", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_many_leaf.json"))
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    assert a.laps or a.parent_lib, "--parent-lib: the baseline is the parent commit's library"
    assert a.laps or a.rounds >= 25, "at least 25 interleaved rounds per shape"

    import torch
    torch.cuda.init()
    kzg = importlib.import_module("rust-eth-kzg_amd")
    lib = kzg.load_library()
    ctx = kzg.DASContext(use_precomp=True)
    parent = None if a.laps else ParentLibrary(a.parent_lib, kzg)
    blobs = random_blobs(N_BLOBS, 7594)
    bl = [blobs[b].tobytes() for b in range(N_BLOBS)]
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(bl)
    assert st == [0] * N_BLOBS
    _, comms = ctx.blob_to_kzg_commitment_batch(bl)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rows = []
    for n_problems, n_cells in shapes:
        problems = shape_problems(n_problems, n_cells, comms, cells, proofs)
        nb, lens, tabs, _keep = ctx._marshal_many(problems)
        ver, stt = (C.c_bool * nb)(), (C.c_int32 * nb)()
        starts = np.arange(nb + 1, dtype=np.uint64) * np.uint64(n_cells)
        dev = [torch.from_numpy(np.frombuffer(b"".join(b"".join(p[k]) for p in problems), dtype=np.uint8).copy()).cuda() for k in (0, 2, 3)]
        d_idx = torch.from_numpy(np.array([i for p in problems for i in p[1]], dtype=np.int64)).cuda()
        torch.cuda.synchronize()
        ptrs = [C.c_void_p(dev[0].data_ptr()), C.c_void_p(d_idx.data_ptr()), C.c_void_p(dev[1].data_ptr()), C.c_void_p(dev[2].data_ptr())]

        def host(flags):
            if flags is None:
                res = lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many(ctx.handle, nb, vp(lens[0]), vp(tabs[0]), vp(lens[1]), vp(tabs[1]), vp(lens[2]),
                                                                       vp(tabs[2]), vp(lens[3]), vp(tabs[3]), ver, stt)
            else:
                res = lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex(ctx.handle, nb, vp(lens[0]), vp(tabs[0]), vp(lens[1]), vp(tabs[1]), vp(lens[2]),
                                                                          vp(tabs[2]), vp(lens[3]), vp(tabs[3]), flags, ver, stt)
            ctx._check(res)

        def device(flags):
            ctx._check(lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex(ctx.handle, nb, vp(starts), *ptrs, flags, ver, stt, None))

        calls = {"many": lambda: host(None), "many_ex_leaf": lambda: host(kzg.VERIFY_LEAF_TRANSCRIPT),
                 "device_leaf": lambda: device(kzg.VERIFY_LEAF_TRANSCRIPT), "device_reference": lambda: device(0)}
        if parent:
            calls["parent_many"] = lambda: parent.many(nb, lens, tabs, ver, stt)

        def checked(kind):
            for b in range(nb):
                ver[b] = False
            t0 = time.perf_counter()
            calls[kind]()
            ms = (time.perf_counter() - t0) * 1e3
            assert all(ver) and not any(stt), kind
            return ms

        kinds = [k for k in KINDS if k in calls]
        for _ in range(3):
            for kind in kinds:
                checked(kind)
        if a.laps:
            for kind in kinds:
                print("[laps] %d x %d %s" % (n_problems, n_cells, kind), file=sys.stderr, flush=True)
                checked(kind)
            continue
        samples = {k: [] for k in kinds}
        for i in range(a.rounds):
            for kind in kinds[i % len(kinds):] + kinds[:i % len(kinds)]:
                samples[kind].append(checked(kind))
        row = {"problems": n_problems, "cells_per_problem": n_cells, "kinds": {k: summary(v) for k, v in samples.items()}}
        p, m, d = row["kinds"]["parent_many"], row["kinds"]["many"], row["kinds"]["device_leaf"]
        row["many_within_parent_spread"] = bool(abs(m["median_ms"] - p["median_ms"]) <= p["p90_ms"] - p["p10_ms"])
        row["device_leaf_faster_than_parent_many"] = bool(d["median_ms"] < p["median_ms"])
        row["parent_many_over_device_leaf"] = p["median_ms"] / d["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del dev, d_idx
    if parent:
        parent.close()
    ctx.close()
    if a.laps:
        return
    doc = {"what": "many-verification, milliseconds per call: the parent commit's _many, this build's _many, _many_ex(leaf), _many_device_ex(leaf), "
                   "_many_device_ex(0); interleaved rounds in one process, default tables",
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "host_threads": os.environ.get("ETH_KZG_AMD_HOST_THREADS", "default"),
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
