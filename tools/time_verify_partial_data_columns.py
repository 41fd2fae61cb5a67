"""Partial data columns: eth_kzg_amd_verify_partial_data_columns_device against the many-verification on the expanded input, and the
dense column call against itself on the parent commit; one process, one GPU, buffers in HBM, the leaf flag.

    python tools/time_verify_partial_data_columns.py --parent-lib PATH [--shapes 128x64:alt+four,8x64:alt] [--rounds 25]
                                                     [--out profiles/verify_partial_data_columns.json]

A shape is COLUMNS x BLOBS and the bitmaps timed on it: `alt` sets every second bit of every column (columns of BLOBS / 2 cells), `four`
sets four bits per column (blobs j, j + 16, j + 32, j + 48 mod BLOBS in column j).  A block of BLOBS different blobs, columns
0 .. COLUMNS - 1, all valid.  Per shape, on default tables, after three warm-up calls of every kind, --rounds interleaved rounds; a round
times every kind once, the order rotating from round to round; host clock around each call (all are synchronous).  Kinds:
  (a) the partial call against the expanded call
    parent_expanded_<mask>  eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex of --parent-lib (a libc_eth_kzg.so built from the parent
                            commit, loaded next to this build's, with a context of its own) on the expanded input: one commitment per cell
    partial_<mask>          eth_kzg_amd_verify_partial_data_columns_device of this build on the packed arrays
  (b) the dense call must not pay for the pair list
    parent_columns          eth_kzg_amd_verify_data_columns_device of --parent-lib, every blob in every column
    columns                 the same symbol of this build
Reported per kind: median, minimum, 10th and 90th percentile in milliseconds.  Every timed call must verify every column.  Written next
to the figures: per mask whether the partial call is FASTER than the expanded call (its median below that call's by more than that call's
own p90 - p10), and whether `columns` lies within the parent's own round-to-round spread (p90 - p10) of the parent's median."""
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


def random_blobs(n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, 4096, 32), dtype=np.uint8)
    a[:, :, 0] &= 0x3F  # < 2^254 < r: canonical field elements
    return a.reshape(n, 131072)


def summary(ms):
    s = sorted(ms)
    pick = lambda q: s[min(len(s) - 1, int(q * len(s)))]  # noqa: E731
    return {"median_ms": statistics.median(s), "min_ms": s[0], "p10_ms": pick(0.10), "p90_ms": pick(0.90), "calls": len(s)}


def bitmap(kind, column, n_blobs):
    if kind == "alt":
        return sum(1 << i for i in range(column % 2, n_blobs, 2))
    assert kind == "four", kind
    return sum(1 << ((column + 16 * k) % n_blobs) for k in range(4))


class ParentLibrary:
    """the parent commit's product library, loaded next to this build's: its own context, its _many_device_ex and its dense column call"""

    def __init__(self, path, kzg):
        self.lib = C.CDLL(os.path.abspath(path))
        P, U64 = C.c_void_p, C.c_uint64
        self.lib.eth_kzg_amd_das_context_new_on_device.restype = P
        self.lib.eth_kzg_amd_das_context_new_on_device.argtypes = [C.c_bool, C.c_int]
        self.lib.eth_kzg_amd_tables_ready.argtypes = [P, C.c_int]
        self.lib.eth_kzg_das_context_free.argtypes = [P]
        self.many_device = self.lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex
        self.many_device.restype = kzg.CResult
        self.many_device.argtypes = [P, U64, P, P, P, P, P, C.c_uint32, P, P, P]
        self.columns_device = self.lib.eth_kzg_amd_verify_data_columns_device
        self.columns_device.restype = kzg.CResult
        self.columns_device.argtypes = [P, U64, P, U64, P, P, P, C.c_uint32, P, P, P]
        assert os.path.realpath(path) != os.path.realpath(kzg.load_library()._name), "--parent-lib is the library under test itself"
        assert not hasattr(self.lib, "eth_kzg_amd_verify_partial_data_columns"), "--parent-lib already has the partial call: not the parent commit's"
        self.ctx = C.c_void_p(self.lib.eth_kzg_amd_das_context_new_on_device(True, 0))
        while self.lib.eth_kzg_amd_tables_ready(self.ctx, 1000) == 0:
            pass

    def close(self):
        self.lib.eth_kzg_das_context_free(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x64:alt+four,8x64:alt")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_partial_data_columns.json"))
    a = ap.parse_args()
    shapes = []
    for s in a.shapes.split(","):
        dims, masks = s.split(":")
        shapes.append(tuple(int(v) for v in dims.split("x")) + (masks.split("+"),))
    assert a.rounds >= 25, "at least 25 interleaved rounds per shape"
    max_blobs = max(nb for _, nb, _ in shapes)

    import torch
    torch.cuda.init()
    kzg = importlib.import_module("rust-eth-kzg_amd")
    lib = kzg.load_library()
    ctx = kzg.DASContext(use_precomp=True)
    parent = ParentLibrary(a.parent_lib, kzg)
    blobs = random_blobs(max_blobs, 7594)
    bl = [blobs[b].tobytes() for b in range(max_blobs)]
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(bl)
    assert st == [0] * max_blobs
    _, comms = ctx.blob_to_kzg_commitment_batch(bl)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    p_ = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    up = lambda raw: torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()  # noqa: E731
    LEAF = kzg.VERIFY_LEAF_TRANSCRIPT
    rows = []
    for n_columns, n_blobs, masks in shapes:
        idx = np.arange(n_columns, dtype=np.uint64)
        ver, stt = (C.c_bool * n_columns)(), (C.c_int32 * n_columns)()
        d_comm = up(b"".join(comms[:n_blobs]))
        d_cells = up(b"".join(cells[b][c] for c in range(n_columns) for b in range(n_blobs)))
        d_proofs = up(b"".join(proofs[b][c] for c in range(n_columns) for b in range(n_blobs)))
        keep, calls = [d_comm, d_cells, d_proofs], {}
        calls["parent_columns"] = lambda: parent.columns_device(parent.ctx, n_blobs, p_(d_comm), n_columns, vp(idx), p_(d_cells), p_(d_proofs), LEAF, ver, stt, None)
        calls["columns"] = lambda: lib.eth_kzg_amd_verify_data_columns_device(ctx.handle, n_blobs, p_(d_comm), n_columns, vp(idx), p_(d_cells),
                                                                              p_(d_proofs), LEAF, ver, stt, None)
        cells_of = {}
        for mask in masks:
            present = [bitmap(mask, c, n_blobs) for c in range(n_columns)]
            held = [[b for b in range(n_blobs) if (present[c] >> b) & 1] for c in range(n_columns)]
            bits, _ = ctx._present_words(n_blobs, present)
            pk_cells = up(b"".join(cells[b][c] for c in range(n_columns) for b in held[c]))
            pk_proofs = up(b"".join(proofs[b][c] for c in range(n_columns) for b in held[c]))
            x_comm = up(b"".join(comms[b] for c in range(n_columns) for b in held[c]))  # the expanded input: one commitment per cell
            x_idx = torch.tensor([c for c in range(n_columns) for _ in held[c]], dtype=torch.int64).cuda()
            starts = np.cumsum([0] + [len(h) for h in held]).astype(np.uint64)
            keep += [bits, pk_cells, pk_proofs, x_comm, x_idx, starts]
            cells_of[mask] = int(starts[-1])
            calls["parent_expanded_" + mask] = (lambda s=starts, xc=x_comm, xi=x_idx, c=pk_cells, p=pk_proofs: parent.many_device(
                parent.ctx, n_columns, vp(s), p_(xc), p_(xi), p_(c), p_(p), LEAF, ver, stt, None))
            calls["partial_" + mask] = (lambda b=bits, c=pk_cells, p=pk_proofs: lib.eth_kzg_amd_verify_partial_data_columns_device(
                ctx.handle, n_blobs, p_(d_comm), n_columns, vp(idx), vp(b), p_(c), p_(p), LEAF, ver, stt, None))
        torch.cuda.synchronize()

        def checked(kind):
            for b in range(n_columns):
                ver[b] = False
            t0 = time.perf_counter()
            res = calls[kind]()
            ms = (time.perf_counter() - t0) * 1e3
            assert res.status == 0, (kind, C.string_at(res.error_msg))
            assert all(ver) and not any(stt), kind
            return ms

        kinds = list(calls)
        for _ in range(3):
            for kind in kinds:
                checked(kind)
        samples = {k: [] for k in kinds}
        for i in range(a.rounds):
            for kind in kinds[i % len(kinds):] + kinds[:i % len(kinds)]:
                samples[kind].append(checked(kind))
        row = {"columns": n_columns, "blobs": n_blobs, "cells": dict(cells_of, dense=n_columns * n_blobs),
               "kinds": {k: summary(v) for k, v in samples.items()}}
        for mask in masks:
            y, c = row["kinds"]["parent_expanded_" + mask], row["kinds"]["partial_" + mask]
            row["partial_%s_over_expanded" % mask] = c["median_ms"] / y["median_ms"]
            row["partial_%s_faster_than_expanded" % mask] = bool(y["median_ms"] - c["median_ms"] > y["p90_ms"] - y["p10_ms"])
        p, m = row["kinds"]["parent_columns"], row["kinds"]["columns"]
        row["parent_columns_spread_ms"] = p["p90_ms"] - p["p10_ms"]
        row["columns_within_parent_spread"] = bool(abs(m["median_ms"] - p["median_ms"]) <= row["parent_columns_spread_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del keep, calls, d_comm, d_cells, d_proofs
    parent.close()
    ctx.close()
    doc = {"what": "partial data columns, milliseconds per call under the leaf flag, buffers in HBM: eth_kzg_amd_verify_partial_data_columns_device "
                   "against the parent commit's _many_device_ex on the expanded input, and eth_kzg_amd_verify_data_columns_device of this build "
                   "against the parent commit's; interleaved rounds in one process, default tables",
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "host_threads": os.environ.get("ETH_KZG_AMD_HOST_THREADS", "default"),
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
