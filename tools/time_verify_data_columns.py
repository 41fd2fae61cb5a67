"""The data columns of one block: eth_kzg_amd_verify_data_columns / _device against the many-verification on the expanded input, one process,
one GPU.

    python tools/time_verify_data_columns.py --parent-lib PATH [--shapes 128x6,128x21,128x64,8x64] [--rounds 25]
                                             [--out profiles/verify_data_columns.json]
    ETH_KZG_AMD_TRACE=1 python tools/time_verify_data_columns.py --laps [--shapes 128x64]

Shapes are COLUMNS x BLOBS: a block of BLOBS different blobs, columns 0 .. COLUMNS - 1, all valid; the expanded input repeats the BLOBS
commitments once per cell (tests/data_columns.py: expand).  Per shape, on default tables, after three warm-up calls of every kind,
--rounds interleaved rounds; a round times every kind once, the order rotating from round to round; host clock around each call (all are
synchronous: they return verdicts).  Kinds:
    parent_many            eth_kzg_amd_verify_cell_kzg_proof_batch_many of --parent-lib (a libc_eth_kzg.so built from the parent commit, loaded
                           next to this build's, with a context of its own) on the expanded input
    many                   the same symbol of this build: the existing call must not have moved
    many_ex_leaf           eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex with the leaf flag, expanded input
    many_device_leaf       eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex with the flag, expanded flat arrays in HBM: THE YARDSTICK
    many_device_reference  the same with flags = 0
    columns, columns_leaf                  eth_kzg_amd_verify_data_columns, flags 0 / leaf, pointer tables marshalled once
    columns_device, columns_device_leaf    eth_kzg_amd_verify_data_columns_device, flags 0 / leaf, arrays resident in HBM
Reported per kind: median, minimum, 10th and 90th percentile in milliseconds.  Every timed call must verify every column.  Written next
to the figures: whether `many` lies within the parent's own spread of the parent's median, and whether columns_device_leaf is FASTER than
many_device_leaf -- which stands only if its median lies below that call's median by more than that call's own p90 - p10.  --laps: no
timing; with ETH_KZG_AMD_TRACE=1 in the environment the library prints the laps of one call of many_device_leaf and of
columns_device_leaf per shape on stderr, behind a line that names the call."""
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
KINDS = ["parent_many", "many", "many_ex_leaf", "many_device_leaf", "many_device_reference", "columns", "columns_leaf", "columns_device",
         "columns_device_leaf"]
LAP_KINDS = ["many_device_leaf", "columns_device_leaf"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x6,128x21,128x64,8x64")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--laps", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_data_columns.json"))
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    assert a.laps or a.parent_lib, "--parent-lib: the existing call is compared with the parent commit's library"
    assert a.laps or a.rounds >= 25, "at least 25 interleaved rounds per shape"
    max_blobs = max(nb for _, nb in shapes)

    import torch
    torch.cuda.init()
    kzg = importlib.import_module("rust-eth-kzg_amd")
    lib = kzg.load_library()
    ctx = kzg.DASContext(use_precomp=True)
    parent = None if a.laps else ParentLibrary(a.parent_lib, kzg)
    blobs = random_blobs(max_blobs, 7594)
    bl = [blobs[b].tobytes() for b in range(max_blobs)]
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(bl)
    assert st == [0] * max_blobs
    _, comms = ctx.blob_to_kzg_commitment_batch(bl)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    LEAF = kzg.VERIFY_LEAF_TRANSCRIPT
    rows = []
    for n_columns, n_blobs in shapes:
        call = (comms[:n_blobs], list(range(n_columns)), [[cells[b][c] for b in range(n_blobs)] for c in range(n_columns)],
                [[proofs[b][c] for b in range(n_blobs)] for c in range(n_columns)])
        problems = [(call[0], [c] * n_blobs, call[2][c], call[3][c]) for c in range(n_columns)]  # the expanded input
        nb, lens, tabs, _keep = ctx._marshal_many(problems)
        _, _, ca, idx, cla, pa, _keep2 = ctx._marshal_columns(*call)
        ver, stt = (C.c_bool * nb)(), (C.c_int32 * nb)()
        up = lambda raw: torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()  # noqa: E731
        d_comm, d_cells, d_proofs = up(b"".join(call[0])), up(b"".join(b"".join(col) for col in call[2])), up(b"".join(b"".join(col) for col in call[3]))
        d_comm_x = d_comm.repeat(n_columns).contiguous()  # the expanded form's commitments: once per cell
        d_idx_x = torch.arange(n_columns, dtype=torch.int64).repeat_interleave(n_blobs).cuda()
        starts = np.arange(nb + 1, dtype=np.uint64) * np.uint64(n_blobs)
        torch.cuda.synchronize()
        p_ = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def many(flags):
            if flags is None:
                res = lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many(ctx.handle, nb, vp(lens[0]), vp(tabs[0]), vp(lens[1]), vp(tabs[1]), vp(lens[2]),
                                                                       vp(tabs[2]), vp(lens[3]), vp(tabs[3]), ver, stt)
            else:
                res = lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex(ctx.handle, nb, vp(lens[0]), vp(tabs[0]), vp(lens[1]), vp(tabs[1]), vp(lens[2]),
                                                                          vp(tabs[2]), vp(lens[3]), vp(tabs[3]), flags, ver, stt)
            ctx._check(res)

        def many_device(flags):
            ctx._check(lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex(ctx.handle, nb, vp(starts), p_(d_comm_x), p_(d_idx_x), p_(d_cells),
                                                                                  p_(d_proofs), flags, ver, stt, None))

        def columns(flags):
            ctx._check(lib.eth_kzg_amd_verify_data_columns(ctx.handle, n_blobs, vp(ca), n_columns, vp(idx), vp(cla), vp(pa), flags, ver, stt))

        def columns_device(flags):
            ctx._check(lib.eth_kzg_amd_verify_data_columns_device(ctx.handle, n_blobs, p_(d_comm), n_columns, vp(idx), p_(d_cells), p_(d_proofs), flags,
                                                                  ver, stt, None))

        calls = {"many": lambda: many(None), "many_ex_leaf": lambda: many(LEAF), "many_device_leaf": lambda: many_device(LEAF),
                 "many_device_reference": lambda: many_device(0), "columns": lambda: columns(0), "columns_leaf": lambda: columns(LEAF),
                 "columns_device": lambda: columns_device(0), "columns_device_leaf": lambda: columns_device(LEAF)}
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
            for kind in LAP_KINDS:
                print("[laps] %d x %d %s" % (n_columns, n_blobs, kind), file=sys.stderr, flush=True)
                checked(kind)
            continue
        samples = {k: [] for k in kinds}
        for i in range(a.rounds):
            for kind in kinds[i % len(kinds):] + kinds[:i % len(kinds)]:
                samples[kind].append(checked(kind))
        row = {"columns": n_columns, "blobs": n_blobs, "kinds": {k: summary(v) for k, v in samples.items()}}
        p, m = row["kinds"]["parent_many"], row["kinds"]["many"]
        y, c = row["kinds"]["many_device_leaf"], row["kinds"]["columns_device_leaf"]
        row["many_within_parent_spread"] = bool(abs(m["median_ms"] - p["median_ms"]) <= p["p90_ms"] - p["p10_ms"])
        row["yardstick_spread_ms"] = y["p90_ms"] - y["p10_ms"]
        row["columns_device_leaf_faster_than_many_device_leaf"] = bool(y["median_ms"] - c["median_ms"] > row["yardstick_spread_ms"])
        row["columns_device_leaf_over_many_device_leaf"] = c["median_ms"] / y["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d_comm, d_cells, d_proofs, d_comm_x, d_idx_x
    if parent:
        parent.close()
    ctx.close()
    if a.laps:
        return
    doc = {"what": "data columns of one block, milliseconds per call: eth_kzg_amd_verify_data_columns / _device under both flags against _many, "
                   "_many_ex(leaf), _many_device_ex(leaf: the yardstick) and _many_device_ex(0) on the expanded input, and the parent commit's _many; "
                   "interleaved rounds in one process, default tables",
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "host_threads": os.environ.get("ETH_KZG_AMD_HOST_THREADS", "default"),
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
