"""A block's data columns recovered and checked against its commitments: eth_kzg_amd_recover_data_columns_checked_device against what a
caller does today with the parent commit's library, one process, one GPU.

    python tools/time_recover_checked.py --parent-lib PATH [--shapes 64x6,64x21,64x64,128x64] [--rounds 25]
                                         [--out profiles/recover_checked.json]

Shapes are COLUMNS x BLOBS: a block of BLOBS different blobs of which COLUMNS columns are held (128: all; otherwise a seeded choice), all
right, everything resident in HBM.  Per shape, on default tables, after three warm-up calls of every kind, --rounds interleaved rounds; a
round times every kind once, the order rotating from round to round; host clock around each call, the device synchronised before the
clock stops.  --parent-lib: a libc_eth_kzg.so built from the parent commit, loaded next to this build's, with a context of its own.  Kinds:
    parent_recover             the parent's eth_kzg_amd_recover_data_columns_device, cells and proofs
    recover                    the same symbol of this build: the existing call must not have moved
    parent_recover_commit      today's careful caller, way two: the parent's recovery, the gather of the recovered cells 0..63 into
                               blob-major order (the caller has to do it: one strided device copy), the parent's
                               eth_kzg_amd_blob_to_kzg_commitment_device on them, and the comparison of the 48-byte records
    checked                    eth_kzg_amd_recover_data_columns_checked_device with commitments, cells and proofs out
    parent_verify_leaf         today's way to learn what the pure check says: the parent's eth_kzg_amd_verify_data_columns_device with the
                               leaf flag on the same columns and their proofs
    pure_check                 the checked call with commitments and no output
Reported per kind: median, minimum, 10th and 90th percentile in milliseconds.  Every timed call must give status 0 everywhere.  Written
next to the figures: whether `recover` lies within the parent's own p10-p90 width of the parent's median, and for the two comparisons
whether the new call is FASTER -- which stands only where the medians differ by more than the two p10-p90 widths added."""
import argparse
import ctypes as C
import importlib
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = ["parent_recover", "recover", "parent_recover_commit", "checked", "parent_verify_leaf", "pure_check"]
BLOB, CELL, PROOF, CELLS = 131072, 2048, 48, 128


def random_blobs(n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, 4096, 32), dtype=np.uint8)
    a[:, :, 0] &= 0x3F  # < 2^254 < r: canonical field elements
    return a.reshape(n, BLOB)


def summary(ms):
    s = sorted(ms)
    pick = lambda q: s[min(len(s) - 1, int(q * len(s)))]  # noqa: E731
    return {"median_ms": statistics.median(s), "min_ms": s[0], "p10_ms": pick(0.10), "p90_ms": pick(0.90), "calls": len(s)}


def width(k):
    return k["p90_ms"] - k["p10_ms"]


class ParentLibrary:
    """the parent commit's product library, loaded next to this build's: its own context and the three calls a caller combines today"""

    def __init__(self, path, kzg):
        self.lib = C.CDLL(os.path.abspath(path))
        P, U64 = C.c_void_p, C.c_uint64
        self.lib.eth_kzg_amd_das_context_new_on_device.restype = P
        self.lib.eth_kzg_amd_das_context_new_on_device.argtypes = [C.c_bool, C.c_int]
        self.lib.eth_kzg_amd_tables_ready.argtypes = [P, C.c_int]
        self.lib.eth_kzg_das_context_free.argtypes = [P]
        for name, args in (("eth_kzg_amd_recover_data_columns_device", [P, U64, U64, P, P, P, P, P, P]),
                           ("eth_kzg_amd_blob_to_kzg_commitment_device", [P, U64, P, P, P, P]),
                           ("eth_kzg_amd_verify_data_columns_device", [P, U64, P, U64, P, P, P, C.c_uint32, P, P, P])):
            getattr(self.lib, name).restype = kzg.CResult
            getattr(self.lib, name).argtypes = args
        assert os.path.realpath(path) != os.path.realpath(kzg.load_library()._name), "--parent-lib is the library under test itself"
        assert not hasattr(self.lib, "eth_kzg_amd_recover_data_columns_checked"), "--parent-lib has the checked call: not the parent commit's"
        self.ctx = C.c_void_p(self.lib.eth_kzg_amd_das_context_new_on_device(True, 0))
        while self.lib.eth_kzg_amd_tables_ready(self.ctx, 1000) == 0:
            pass

    def ok(self, res):
        assert res.status == 0, C.string_at(res.error_msg)

    def close(self):
        self.lib.eth_kzg_das_context_free(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x6,64x21,64x64,128x64")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recover_checked.json"))
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    assert a.rounds >= 25, "at least 25 interleaved rounds per shape"
    max_blobs = max(nb for _, nb in shapes)

    import torch
    torch.cuda.init()
    kzg = importlib.import_module("rust-eth-kzg_amd")
    ctx = kzg.DASContext(use_precomp=True)
    parent = ParentLibrary(a.parent_lib, kzg)
    d_blobs = torch.from_numpy(random_blobs(max_blobs, 7594)).cuda()
    blk_comm = torch.zeros(max_blobs, PROOF, dtype=torch.uint8, device="cuda")
    blk_cells = torch.zeros(CELLS, max_blobs, CELL, dtype=torch.uint8, device="cuda")
    blk_proofs = torch.zeros(CELLS, max_blobs, PROOF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.compute_data_columns_device(max_blobs, d_blobs.data_ptr(), blk_comm.data_ptr(), blk_cells.data_ptr(), blk_proofs.data_ptr()) == [0] * max_blobs
    torch.cuda.synchronize()
    p_ = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    LEAF = kzg.VERIFY_LEAF_TRANSCRIPT
    rows = []
    for n_columns, n in shapes:
        held = list(range(CELLS)) if n_columns == CELLS else sorted(random.Random("recover-checked:%d" % n_columns).sample(range(CELLS), n_columns))
        pick = torch.tensor(held, device="cuda")
        d_in = blk_cells[pick][:, :n].contiguous()         # [n_columns][n][2048]
        d_in_proofs = blk_proofs[pick][:, :n].contiguous()
        d_comm = blk_comm[:n].contiguous()
        idx = np.array(held, dtype=np.uint64)
        out_cells = torch.zeros(CELLS, n, CELL, dtype=torch.uint8, device="cuda")
        out_proofs = torch.zeros(CELLS, n, PROOF, dtype=torch.uint8, device="cuda")
        rec_comm = torch.zeros(n, PROOF, dtype=torch.uint8, device="cuda")
        st, st2 = (C.c_int32 * n)(), (C.c_int32 * n)()
        ver, vst = (C.c_bool * n_columns)(), (C.c_int32 * n_columns)()
        torch.cuda.synchronize()

        def parent_recover():
            parent.ok(parent.lib.eth_kzg_amd_recover_data_columns_device(parent.ctx, n, n_columns, idx.ctypes.data_as(C.c_void_p), p_(d_in), p_(out_cells),
                                                                         p_(out_proofs), st, None))
            return list(st)

        def recover():
            return ctx.recover_data_columns_device(n, held, d_in.data_ptr(), out_cells.data_ptr(), out_proofs.data_ptr())

        def parent_recover_commit():
            s = parent_recover()
            gathered = out_cells[:CELLS // 2].permute(1, 0, 2).contiguous()  # [n][64][2048]: the recovered blobs, blob-major
            torch.cuda.synchronize()  # (the commitment call below runs behind the default stream; the copy ran on torch's current one)
            parent.ok(parent.lib.eth_kzg_amd_blob_to_kzg_commitment_device(parent.ctx, n, p_(gathered), p_(rec_comm), st2, None))
            assert bool(torch.equal(rec_comm, d_comm))  # the comparison the caller is after
            return [x or y for x, y in zip(s, st2)]

        def checked():
            return ctx.recover_data_columns_checked_device(n, held, d_in.data_ptr(), d_comm.data_ptr(), d_out_cells=out_cells.data_ptr(),
                                                           d_out_proofs=out_proofs.data_ptr())

        def parent_verify_leaf():
            parent.ok(parent.lib.eth_kzg_amd_verify_data_columns_device(parent.ctx, n, p_(d_comm), n_columns, idx.ctypes.data_as(C.c_void_p), p_(d_in),
                                                                        p_(d_in_proofs), LEAF, ver, vst, None))
            assert all(ver) and not any(vst)
            return [0] * n

        def pure_check():
            return ctx.recover_data_columns_checked_device(n, held, d_in.data_ptr(), d_comm.data_ptr())

        calls = {"parent_recover": parent_recover, "recover": recover, "parent_recover_commit": parent_recover_commit, "checked": checked,
                 "parent_verify_leaf": parent_verify_leaf, "pure_check": pure_check}

        def timed(kind):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            status = calls[kind]()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            assert status == [0] * n, (kind, status)
            return ms

        for _ in range(3):
            for kind in KINDS:
                timed(kind)
        samples = {k: [] for k in KINDS}
        for i in range(a.rounds):
            for kind in KINDS[i % len(KINDS):] + KINDS[:i % len(KINDS)]:
                samples[kind].append(timed(kind))
        k = {name: summary(v) for name, v in samples.items()}
        row = {"columns": n_columns, "blobs": n, "kinds": k}
        row["recover_within_parent_spread"] = bool(abs(k["recover"]["median_ms"] - k["parent_recover"]["median_ms"]) <= width(k["parent_recover"]))
        for new, old in (("checked", "parent_recover_commit"), ("pure_check", "parent_verify_leaf")):
            row["%s_faster_than_%s" % (new, old)] = bool(k[old]["median_ms"] - k[new]["median_ms"] > width(k[old]) + width(k[new]))
            row["%s_over_%s" % (new, old)] = k[new]["median_ms"] / k[old]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    parent.close()
    ctx.close()
    doc = {"what": "checked recovery of a block's data columns, milliseconds per call, everything resident in HBM: "
                   "eth_kzg_amd_recover_data_columns_checked_device (cells + proofs; pure check) against the parent commit's recover_data_columns_device "
                   "+ gather + blob_to_kzg_commitment_device and against its verify_data_columns_device(leaf); this build's recover_data_columns_device "
                   "against the parent's; interleaved rounds in one process, default tables",
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
