"""A block's data columns computed and recovered in column layout: eth_kzg_amd_compute_data_columns_device and
eth_kzg_amd_recover_data_columns_device against what a caller does without them -- the blob-major calls of the PARENT commit's library
plus torch permutes into and out of the column layout -- one process, one GPU, buffers resident in HBM.

    python tools/time_data_columns.py --parent-lib PATH [--blobs 6,21,64,128] [--rounds 25] [--out profiles/data_columns.json]
    python tools/time_data_columns.py --recover-only this|parent [--parent-lib PATH] [--blobs 64] [--calls 20]     (under rocprofv3)

Per block size, on default tables, after three warm-up calls of every kind, --rounds interleaved rounds; a round times every kind once,
the order rotating from round to round; host clock around work that ends in a device synchronise.  Kinds:
    columns                 eth_kzg_amd_compute_data_columns_device: commitments, cells and proofs of the block, column layout
    parent_pair_permute     the parent library's blob_to_kzg_commitment_device + compute_cells_and_kzg_proofs_device, then cells and proofs
                            permuted into [128][n] by torch: THE YARDSTICK of the prover
    pair_permute            the same three steps on this build
    cells_proofs            this build's blob-major compute_cells_and_kzg_proofs_device alone, and
    parent_cells_proofs     the parent's: the existing call must not have moved (also timed at --also-blob-major sizes, 64 and 2048)
    recover_columns         eth_kzg_amd_recover_data_columns_device from the 64 even columns
    parent_recover_permute  the held columns scattered into [n][128][2048] by torch, the parent's recover_cells_and_proofs_device with a mask
                            per blob, cells and proofs permuted back: THE YARDSTICK of recovery
Reported per kind: median, minimum, 10th and 90th percentile in milliseconds; every output is compared byte for byte once, before the
timing.  A column call counts as faster (slower) than its yardstick only if the medians differ by more than the yardstick's own
p90 - p10.  --recover-only: no timing -- --calls recoveries of one kind at one size on the start tables, for a kernel trace."""
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
BLOB, CELL, PROOF, CELLS = 131072, 2048, 48, 128
HELD = list(range(0, 128, 2))


def random_blobs(n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, 4096, 32), dtype=np.uint8)
    a[:, :, 0] &= 0x3F  # < 2^254 < r: canonical field elements
    return a.reshape(n, BLOB)


def summary(ms):
    s = sorted(ms)
    pick = lambda q: s[min(len(s) - 1, int(q * len(s)))]  # noqa: E731
    return {"median_ms": statistics.median(s), "min_ms": s[0], "p10_ms": pick(0.10), "p90_ms": pick(0.90), "calls": len(s)}


class ParentLibrary:
    """the parent commit's product library, loaded next to this build's, with a context of its own: its three blob-major device calls"""

    def __init__(self, path, kzg):
        self.lib = C.CDLL(os.path.abspath(path))
        P, U64 = C.c_void_p, C.c_uint64
        self.lib.eth_kzg_amd_das_context_new_on_device.restype = P
        self.lib.eth_kzg_amd_das_context_new_on_device.argtypes = [C.c_bool, C.c_int]
        self.lib.eth_kzg_amd_tables_ready.argtypes = [P, C.c_int]
        self.lib.eth_kzg_das_context_free.argtypes = [P]
        for name, args in {"eth_kzg_amd_blob_to_kzg_commitment_device": [P, U64, P, P, P, P],
                           "eth_kzg_amd_compute_cells_and_kzg_proofs_device": [P, U64, P, P, P, P, P],
                           "eth_kzg_amd_recover_cells_and_proofs_device": [P, U64, P, P, P, P, P, P]}.items():
            getattr(self.lib, name).restype = kzg.CResult
            getattr(self.lib, name).argtypes = args
        assert not hasattr(self.lib, "eth_kzg_amd_compute_data_columns"), "--parent-lib has the column calls: it is not the parent's build"
        self.ctx = C.c_void_p(self.lib.eth_kzg_amd_das_context_new_on_device(True, 0))
        while self.lib.eth_kzg_amd_tables_ready(self.ctx, 1000) == 0:
            pass

    def _ok(self, res):
        assert res.status == 0, C.string_at(res.error_msg)

    def commit(self, n, d_blobs, d_out, st):
        self._ok(self.lib.eth_kzg_amd_blob_to_kzg_commitment_device(self.ctx, n, d_blobs, d_out, st, None))

    def cells_proofs(self, n, d_blobs, d_cells, d_proofs, st):
        self._ok(self.lib.eth_kzg_amd_compute_cells_and_kzg_proofs_device(self.ctx, n, d_blobs, d_cells, d_proofs, st, None))

    def recover(self, n, d_cells, masks, d_out_cells, d_out_proofs, st):
        self._ok(self.lib.eth_kzg_amd_recover_cells_and_proofs_device(self.ctx, n, d_cells, masks.ctypes.data_as(C.c_void_p), d_out_cells, d_out_proofs, st, None))

    def close(self):
        self.lib.eth_kzg_das_context_free(self.ctx)


class ThisLibrary:
    """the same three calls of this build, under the same method names"""

    def __init__(self, kzg, ctx):
        self.lib, self.ctx, self.check = kzg.load_library(), ctx.handle, ctx._check

    def commit(self, n, d_blobs, d_out, st):
        self.check(self.lib.eth_kzg_amd_blob_to_kzg_commitment_device(self.ctx, n, d_blobs, d_out, st, None))

    def cells_proofs(self, n, d_blobs, d_cells, d_proofs, st):
        self.check(self.lib.eth_kzg_amd_compute_cells_and_kzg_proofs_device(self.ctx, n, d_blobs, d_cells, d_proofs, st, None))

    def recover(self, n, d_cells, masks, d_out_cells, d_out_proofs, st):
        self.check(self.lib.eth_kzg_amd_recover_cells_and_proofs_device(self.ctx, n, d_cells, masks.ctypes.data_as(C.c_void_p), d_out_cells, d_out_proofs, st, None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blobs", default="6,21,64,128")
    ap.add_argument("--also-blob-major", default="64,2048", help="sizes at which only cells_proofs / parent_cells_proofs are timed")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--recover-only", choices=["this", "parent"], default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--parent-commit", default="", help="recorded in the output: the commit --parent-lib was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_columns.json"))
    a = ap.parse_args()
    sizes = [int(v) for v in a.blobs.split(",")]
    extra = [int(v) for v in a.also_blob_major.split(",") if v] if not a.recover_only else []
    assert a.recover_only or a.parent_lib, "--parent-lib: the yardstick is the parent commit's library"
    assert a.recover_only or a.rounds >= 25, "at least 25 interleaved rounds per size"
    if a.recover_only:
        os.environ.setdefault("ETH_KZG_AMD_TABLE_GB", "3")  # the start tables: the decoder does not read them

    import torch
    torch.cuda.init()
    kzg = importlib.import_module("rust-eth-kzg_amd")
    ctx = kzg.DASContext(use_precomp=True)
    this = ThisLibrary(kzg, ctx)
    parent = ParentLibrary(a.parent_lib, kzg) if a.parent_lib and a.recover_only != "this" else None
    p_ = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    dev = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device="cuda")  # noqa: E731
    held = torch.tensor(HELD, device="cuda")
    rows = []
    for n in sizes + [x for x in extra if x not in sizes]:
        blob_major_only = n not in sizes
        d_blobs = torch.from_numpy(random_blobs(n, 7594 + n)).cuda()
        st = (C.c_int32 * n)()
        bm_cells, bm_proofs, bm_comm = dev(n, CELLS, CELL), dev(n, CELLS, PROOF), dev(n, PROOF)
        col_cells, col_proofs, col_comm = dev(CELLS, n, CELL), dev(CELLS, n, PROOF), dev(n, PROOF)
        out_cells, out_proofs = dev(CELLS, n, CELL), dev(CELLS, n, PROOF)
        masks = kzg.present_masks(n, [HELD] * n)
        torch.cuda.synchronize()

        def pair_permute(lib):
            lib.commit(n, p_(d_blobs), p_(bm_comm), st)
            lib.cells_proofs(n, p_(d_blobs), p_(bm_cells), p_(bm_proofs), st)
            out_cells.copy_(bm_cells.permute(1, 0, 2))
            out_proofs.copy_(bm_proofs.permute(1, 0, 2))

        def columns():
            ctx._check(this.lib.eth_kzg_amd_compute_data_columns_device(ctx.handle, n, p_(d_blobs), p_(col_comm), p_(col_cells), p_(col_proofs), st, None))

        def recover_columns():
            ctx._check(this.lib.eth_kzg_amd_recover_data_columns_device(ctx.handle, n, len(HELD), held_idx.ctypes.data_as(C.c_void_p), p_(d_held),
                                                                        p_(out_cells), p_(out_proofs), st, None))

        def recover_permute(lib):
            bm_cells[:, held] = d_held.permute(1, 0, 2)  # un-transpose what the node holds; the other cells are never read
            lib.recover(n, p_(bm_cells), masks, p_(bm_cells2), p_(bm_proofs), st)
            out_cells.copy_(bm_cells2.permute(1, 0, 2))
            out_proofs.copy_(bm_proofs.permute(1, 0, 2))

        calls = {"cells_proofs": lambda: this.cells_proofs(n, p_(d_blobs), p_(bm_cells), p_(bm_proofs), st)}
        if parent:
            calls["parent_cells_proofs"] = lambda: parent.cells_proofs(n, p_(d_blobs), p_(bm_cells), p_(bm_proofs), st)
        if not blob_major_only:
            # the block once, column layout, and every kind against it byte for byte
            columns()
            torch.cuda.synchronize()
            assert not any(st)
            d_held = col_cells[held].contiguous()
            held_idx = np.array(HELD, dtype=np.uint64)
            bm_cells2 = dev(n, CELLS, CELL)
            calls.update({"columns": columns, "pair_permute": lambda: pair_permute(this), "recover_columns": recover_columns})
            if parent:
                calls.update({"parent_pair_permute": lambda: pair_permute(parent), "parent_recover_permute": lambda: recover_permute(parent)})
            if a.recover_only:
                calls = {"this": recover_columns, "parent": (lambda: recover_permute(parent)) if parent else None}
                for _ in range(a.calls):
                    calls[a.recover_only]()
                    torch.cuda.synchronize()
                    assert not any(st) and torch.equal(out_cells, col_cells) and torch.equal(out_proofs, col_proofs)
                continue
            for kind in [k for k in calls if k.endswith("permute") or k == "recover_columns"]:
                out_cells.zero_()
                out_proofs.zero_()
                calls[kind]()
                torch.cuda.synchronize()
                assert not any(st) and torch.equal(out_cells, col_cells) and torch.equal(out_proofs, col_proofs), kind
                assert "recover" in kind or torch.equal(bm_comm, col_comm), kind

        def timed(kind):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls[kind]()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        kinds = list(calls)
        for _ in range(3):
            for kind in kinds:
                timed(kind)
        samples = {k: [] for k in kinds}
        for i in range(a.rounds):
            for kind in kinds[i % len(kinds):] + kinds[:i % len(kinds)]:
                samples[kind].append(timed(kind))
        row = {"blobs": n, "kinds": {k: summary(v) for k, v in samples.items()}}
        k = row["kinds"]

        def against(call, yardstick):
            spread = k[yardstick]["p90_ms"] - k[yardstick]["p10_ms"]
            diff = k[call]["median_ms"] - k[yardstick]["median_ms"]
            return {"yardstick_spread_ms": spread, "median_difference_ms": diff, "verdict": "faster" if -diff > spread else "slower" if diff > spread else "within the spread"}

        if parent:
            row["cells_proofs_against_parent"] = against("cells_proofs", "parent_cells_proofs")
            if not blob_major_only:
                row["columns_against_parent_pair_permute"] = against("columns", "parent_pair_permute")
                row["recover_columns_against_parent_recover_permute"] = against("recover_columns", "parent_recover_permute")
        rows.append(row)
        print(json.dumps(row), flush=True)
    if parent:
        parent.close()
    ctx.close()
    if a.recover_only:
        return
    doc = {"what": "a block's data columns, milliseconds per call ending in a device synchronise: eth_kzg_amd_compute_data_columns_device and "
                   "eth_kzg_amd_recover_data_columns_device (64 even columns held) against the parent commit's blob-major device calls plus torch "
                   "permutes into and out of the column layout; interleaved rounds in one process, default tables, buffers resident in HBM",
           "parent_commit": a.parent_commit, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
