"""Many blobs against their 128 cell proofs per call, a verdict each, against what a caller does today; one process, one GPU.

    python tools/time_verify_blob_cell_proofs.py --parent-lib PATH [--shapes 6,64,1024] [--rounds 25]
                                                 [--out profiles/verify_blob_cell_proofs.json]
    ETH_KZG_AMD_TRACE=1 python tools/time_verify_blob_cell_proofs.py --laps [--shapes 64]

Items are N valid (blob, commitment, 128 cell proofs) of N distinct random blobs (commitments and proofs from the device forms of this
build's prover); the host forms' pointer tables are marshalled once, the device forms' arrays are resident in HBM.  Per shape, on
default tables, after three warm-up calls of every kind, --rounds interleaved rounds; a round times every kind once, the order rotating
from round to round; host clock around each call (all are synchronous: they return verdicts).  Kinds:
    parent_host    on --parent-lib (a libc_eth_kzg.so built from the parent commit, loaded next to this build's, with a context of its
                   own): eth_kzg_amd_compute_cells_and_kzg_proofs_batch with the proofs skipped, then
                   eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex with the leaf flag on the expanded input (128 pointers to the
                   commitment and the indices 0..127 per item, built once, outside the clock)
    parent_device  the same on resident arrays: eth_kzg_amd_compute_cells_and_kzg_proofs_device with the proofs skipped, then
                   eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex with the leaf flag (the expanded commitments and indices
                   resident as well, built once)
    host           eth_kzg_amd_verify_blob_cell_proofs_many of this build
    device         eth_kzg_amd_verify_blob_cell_proofs_many_device of this build
Reported per kind: median, minimum, 10th and 90th percentile in milliseconds.  EVERY timed call's verdicts are checked.  Nothing is gated:
the ratios are written next to the figures, and `*_slower_beyond_parent_spread` says where the new call's median lies above the parent's
by more than the parent's p10-p90.  A second pass per shape plants ONE wrong proof in the middle item and times the new calls again (the
search).  --laps: no timing; with ETH_KZG_AMD_TRACE=1 the library prints the laps of one call of host / device per shape on stderr."""
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
KINDS = ["parent_host", "parent_device", "host", "device"]
BLOB, CELL, N_CELLS, LEAF = 131072, 2048, 128, 1


def random_blobs(n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, 4096, 32), dtype=np.uint8)
    a[:, :, 0] &= 0x3F  # < 2^254 < r: canonical field elements
    return a.reshape(n, BLOB)


def summary(ms):
    s = sorted(ms)
    pick = lambda q: s[min(len(s) - 1, int(q * len(s)))]  # noqa: E731
    return {"median_ms": statistics.median(s), "min_ms": s[0], "p10_ms": pick(0.10), "p90_ms": pick(0.90), "calls": len(s)}


def table(base, count, stride):
    """`count` addresses from `base` on, `stride` bytes apart: a pointer table"""
    return np.uint64(base) + np.arange(max(1, count), dtype=np.uint64) * np.uint64(stride)


class ParentLibrary:
    """the parent commit's product library, loaded next to this build's: its own context and the four calls of today's road"""

    def __init__(self, path, kzg):
        self.lib = C.CDLL(os.path.abspath(path))
        P, U64 = C.c_void_p, C.c_uint64
        self.lib.eth_kzg_amd_das_context_new_on_device.restype = P
        self.lib.eth_kzg_amd_das_context_new_on_device.argtypes = [C.c_bool, C.c_int]
        self.lib.eth_kzg_amd_tables_ready.argtypes = [P, C.c_int]
        self.lib.eth_kzg_das_context_free.argtypes = [P]
        for name, args in {"eth_kzg_amd_compute_cells_and_kzg_proofs_batch": [P, U64, P, P, P, P],
                           "eth_kzg_amd_compute_cells_and_kzg_proofs_device": [P, U64, P, P, P, P, P],
                           "eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex": [P, U64, P, P, P, P, P, P, P, P, C.c_uint32, P, P],
                           "eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex": [P, U64, P, P, P, P, P, C.c_uint32, P, P, P]}.items():
            getattr(self.lib, name).restype = kzg.CResult
            getattr(self.lib, name).argtypes = args
        assert os.path.realpath(path) != os.path.realpath(kzg.load_library()._name), "--parent-lib is the library under test itself"
        assert not hasattr(self.lib, "eth_kzg_amd_verify_blob_cell_proofs_many"), "--parent-lib already has the call under test"
        self.ctx = C.c_void_p(self.lib.eth_kzg_amd_das_context_new_on_device(True, 0))
        while self.lib.eth_kzg_amd_tables_ready(self.ctx, 1000) == 0:
            pass

    def close(self):
        self.lib.eth_kzg_das_context_free(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="6,64,1024")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--laps", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_blob_cell_proofs.json"))
    a = ap.parse_args()
    shapes = [int(s) for s in a.shapes.split(",")]
    assert a.laps or a.parent_lib, "--parent-lib: the baseline is the parent commit's library"

    import torch
    torch.cuda.init()
    kzg = importlib.import_module("rust-eth-kzg_amd")
    lib = kzg.load_library()
    ctx = kzg.DASContext(use_precomp=True)
    parent = None if a.laps else ParentLibrary(a.parent_lib, kzg)
    top = max(shapes)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    dp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    # the material, once, on the device: commitments and the 128 proofs of every blob
    h_blobs = random_blobs(top, 7594)
    d_blobs = torch.from_numpy(h_blobs).cuda()
    d_comm = torch.empty(top * 48, dtype=torch.uint8, device="cuda")
    d_cells = torch.empty(top * N_CELLS * CELL, dtype=torch.uint8, device="cuda")  # (the baseline's cells land here again and again)
    d_good = torch.empty(top * N_CELLS * 48, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st_all = (C.c_int32 * top)()
    ctx._check(lib.eth_kzg_amd_blob_to_kzg_commitment_device(ctx.handle, top, dp(d_blobs), dp(d_comm), st_all, None))
    assert not any(st_all)
    ctx._check(lib.eth_kzg_amd_compute_cells_and_kzg_proofs_device(ctx.handle, top, dp(d_blobs), None, dp(d_good), st_all, None))
    assert not any(st_all)
    h_comm = d_comm.cpu().numpy()
    h_good = d_good.cpu().numpy()
    h_cells = np.zeros(top * N_CELLS * CELL, dtype=np.uint8)  # where the baseline's host form writes its cells
    rows = []
    for n in shapes:
        for wrong in ([], [n // 2]):
            h_proofs = h_good[:n * N_CELLS * 48].copy()
            for i in wrong:  # the proof of cell 5 of the next item
                j = (i + 1) % n
                h_proofs[(i * N_CELLS + 5) * 48:(i * N_CELLS + 6) * 48] = h_good[(j * N_CELLS + 5) * 48:(j * N_CELLS + 6) * 48]
            want = [i not in wrong for i in range(n)]
            d_proofs = torch.from_numpy(h_proofs).cuda()
            # this build's host form: blobs**, commitments**, proofs***
            t_blobs, t_comm = table(h_blobs.ctypes.data, n, BLOB), table(h_comm.ctypes.data, n, 48)
            t_pin = table(h_proofs.ctypes.data, n * N_CELLS, 48)
            t_proofs = table(t_pin.ctypes.data, n, N_CELLS * 8)
            # today's road, expanded once: per item 128 pointers to its commitment, the indices 0..127, pointers to its 128 cells
            t_cin = table(h_cells.ctypes.data, n * N_CELLS, CELL)
            t_cells = table(t_cin.ctypes.data, n, N_CELLS * 8)
            t_kin = np.repeat(t_comm[:n], N_CELLS)
            t_k = table(t_kin.ctypes.data, n, N_CELLS * 8)
            idx = np.tile(np.arange(N_CELLS, dtype=np.uint64), n)
            t_idx = table(idx.ctypes.data, n, N_CELLS * 8)
            lens = np.full(max(1, n), N_CELLS, dtype=np.uint64)
            starts = np.arange(n + 1, dtype=np.uint64) * np.uint64(N_CELLS)
            d_kexp = d_comm[:n * 48].view(n, 1, 48).expand(n, N_CELLS, 48).contiguous()
            d_idx = torch.from_numpy(idx.view(np.int64)).cuda()
            torch.cuda.synchronize()
            ver, stt = (C.c_bool * n)(), (C.c_int32 * n)()

            def parent_host():
                L, h = parent.lib, parent.ctx
                ctx._check(L.eth_kzg_amd_compute_cells_and_kzg_proofs_batch(h, n, vp(t_blobs), vp(t_cells), None, stt))
                assert not any(stt)
                ctx._check(L.eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex(h, n, vp(lens), vp(t_k), vp(lens), vp(t_idx), vp(lens), vp(t_cells), vp(lens),
                                                                             vp(t_proofs), LEAF, ver, stt))

            def parent_device():
                L, h = parent.lib, parent.ctx
                ctx._check(L.eth_kzg_amd_compute_cells_and_kzg_proofs_device(h, n, dp(d_blobs), dp(d_cells), None, stt, None))
                assert not any(stt)
                ctx._check(L.eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex(h, n, vp(starts), dp(d_kexp), dp(d_idx), dp(d_cells), dp(d_proofs), LEAF,
                                                                                    ver, stt, None))

            calls = {"host": lambda: ctx._check(lib.eth_kzg_amd_verify_blob_cell_proofs_many(ctx.handle, n, vp(t_blobs), vp(t_comm), vp(t_proofs), ver, stt)),
                     "device": lambda: ctx._check(lib.eth_kzg_amd_verify_blob_cell_proofs_many_device(ctx.handle, n, dp(d_blobs), dp(d_comm), dp(d_proofs),
                                                                                                      ver, stt, None))}
            if parent and not wrong:
                calls.update({"parent_host": parent_host, "parent_device": parent_device})

            def checked(kind):
                for i in range(n):
                    ver[i] = False
                    stt[i] = 0
                t0 = time.perf_counter()
                calls[kind]()
                ms = (time.perf_counter() - t0) * 1e3
                assert list(ver) == want and not any(stt), (kind, n, wrong)
                return ms

            kinds = [k for k in KINDS if k in calls]
            for _ in range(3):
                for kind in kinds:
                    checked(kind)
            if a.laps:
                for kind in ("host", "device"):
                    print("[laps] %d wrong=%s %s" % (n, wrong, kind), file=sys.stderr, flush=True)
                    checked(kind)
                continue
            samples = {k: [] for k in kinds}
            for i in range(a.rounds):
                for kind in kinds[i % len(kinds):] + kinds[:i % len(kinds)]:
                    samples[kind].append(checked(kind))
            row = {"items": n, "wrong_items": len(wrong), "kinds": {k: summary(v) for k, v in samples.items()}}
            k = row["kinds"]
            for new, old in (("host", "parent_host"), ("device", "parent_device")):
                if old in k:
                    row["%s_over_%s" % (old, new)] = k[old]["median_ms"] / k[new]["median_ms"]
                    row["%s_slower_beyond_parent_spread" % new] = bool(k[new]["median_ms"] - k[old]["median_ms"] > k[old]["p90_ms"] - k[old]["p10_ms"])
            rows.append(row)
            print(json.dumps(row), flush=True)
            del d_proofs, d_kexp, d_idx
    if parent:
        parent.close()
    ctx.close()
    if a.laps:
        return
    doc = {"what": "a blob against its 128 cell proofs, many per call, milliseconds per call: the parent commit's road (cells with the proofs "
                   "skipped, then the many-verification with the leaf flag on the expanded input; host and device form) against "
                   "eth_kzg_amd_verify_blob_cell_proofs_many / _many_device (a verdict each); interleaved rounds in one process, default "
                   "tables; wrong_items = 1: the search for one planted wrong proof",
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "host_threads": os.environ.get("ETH_KZG_AMD_HOST_THREADS", "default"),
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
