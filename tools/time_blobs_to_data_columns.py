"""A block's data columns from blobs whose cell proofs the caller holds, against what a caller composes without the call; one process, one GPU.

    python tools/time_blobs_to_data_columns.py [--shapes 6,21,64] [--rounds 25] [--out profiles/blobs_to_data_columns.json]

Items are N valid (blob, commitment, 128 cell proofs) of N distinct random blobs (commitments and proofs from the device forms of the
prover); the host forms' pointer tables are marshalled once, the device forms' arrays are resident in HBM.  Per shape, on default tables,
after three warm-up calls of every kind, --rounds interleaved rounds; a round times every kind once, the order rotating from round to
round; host clock around work that has completed when the clock stops (the device kinds end in a device synchronise).  Kinds:
    compose_host      eth_kzg_amd_compute_data_columns with out_cells alone, then the proofs transposed [n][128][48] -> [128][n][48] on the host
    new_host          eth_kzg_amd_blobs_to_data_columns, flags = 0
    compose_device    eth_kzg_amd_compute_data_columns_device with d_out_cells alone, then a permute of the resident proofs
    new_device        eth_kzg_amd_blobs_to_data_columns_device, flags = 0
    compose_host_v    compose_host, then eth_kzg_amd_verify_blob_cell_proofs_many
    new_host_v        eth_kzg_amd_blobs_to_data_columns with ETH_KZG_AMD_COLUMNS_VERIFY_PROOFS
    compose_device_v  compose_device, then eth_kzg_amd_verify_blob_cell_proofs_many_device
    new_device_v      eth_kzg_amd_blobs_to_data_columns_device with the flag
The composed calls are the ones a caller has without this call; they run on this build's library, which does not change them.  Every
kind's outputs are compared byte for byte with the composition's before the timing, and every timed call's verdicts are checked.
Nothing is gated: `*_slower_beyond_compose_spread` says where the new call's median lies above the composition's by more than the
composition's own p10-p90."""
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
PAIRS = [("new_host", "compose_host"), ("new_device", "compose_device"), ("new_host_v", "compose_host_v"), ("new_device_v", "compose_device_v")]
BLOB, CELL, N_CELLS, VERIFY = 131072, 2048, 128, 1


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="6,21,64")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blobs_to_data_columns.json"))
    a = ap.parse_args()
    shapes = [int(s) for s in a.shapes.split(",")]

    import torch
    torch.cuda.init()
    kzg = importlib.import_module("rust-eth-kzg_amd")
    lib = kzg.load_library()
    ctx = kzg.DASContext(use_precomp=True)
    while lib.eth_kzg_amd_tables_ready(ctx.handle, 1000) == 0:
        pass
    top = max(shapes)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    dp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    h_blobs = random_blobs(top, 7594)
    d_blobs_all = torch.from_numpy(h_blobs).cuda()
    d_comm_all = torch.empty(top * 48, dtype=torch.uint8, device="cuda")
    d_good = torch.empty(top * N_CELLS * 48, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st_all = (C.c_int32 * top)()
    ctx._check(lib.eth_kzg_amd_blob_to_kzg_commitment_device(ctx.handle, top, dp(d_blobs_all), dp(d_comm_all), st_all, None))
    ctx._check(lib.eth_kzg_amd_compute_cells_and_kzg_proofs_device(ctx.handle, top, dp(d_blobs_all), None, dp(d_good), st_all, None))
    assert not any(st_all)
    h_comm, h_good = d_comm_all.cpu().numpy(), d_good.cpu().numpy()
    rows = []
    for n in shapes:
        h_proofs = h_good[:n * N_CELLS * 48].copy()
        d_blobs, d_comm, d_proofs = d_blobs_all[:n * BLOB], d_comm_all[:n * 48], torch.from_numpy(h_proofs).cuda()
        t_blobs, t_comm = table(h_blobs.ctypes.data, n, BLOB), table(h_comm.ctypes.data, n, 48)
        t_pin = table(h_proofs.ctypes.data, n * N_CELLS, 48)
        t_proofs = table(t_pin.ctypes.data, n, N_CELLS * 8)
        # host outputs [128][n]: one pair of buffers per road, so that the roads can be compared
        out = {}
        for road in ("compose", "new"):
            cells, proofs = np.zeros(N_CELLS * n * CELL, dtype=np.uint8), np.zeros(N_CELLS * n * 48, dtype=np.uint8)
            ci, pi = table(cells.ctypes.data, N_CELLS * n, CELL), table(proofs.ctypes.data, N_CELLS * n, 48)
            out[road] = (cells, proofs, ci, pi, table(ci.ctypes.data, N_CELLS, n * 8), table(pi.ctypes.data, N_CELLS, n * 8))
        d_out = {road: (torch.zeros(N_CELLS * n * CELL, dtype=torch.uint8, device="cuda"), torch.zeros(N_CELLS * n * 48, dtype=torch.uint8, device="cuda"))
                 for road in ("compose", "new")}
        torch.cuda.synchronize()
        ver, stt = (C.c_bool * n)(), (C.c_int32 * n)()

        def compose_host():
            ctx._check(lib.eth_kzg_amd_compute_data_columns(ctx.handle, n, vp(t_blobs), None, vp(out["compose"][4]), None, stt))
            out["compose"][1][:] = h_proofs.reshape(n, N_CELLS, 48).transpose(1, 0, 2).reshape(-1)

        def compose_device():
            ctx._check(lib.eth_kzg_amd_compute_data_columns_device(ctx.handle, n, dp(d_blobs), None, dp(d_out["compose"][0]), None, stt, None))
            d_out["compose"][1].view(N_CELLS, n, 48).copy_(d_proofs.view(n, N_CELLS, 48).permute(1, 0, 2))
            torch.cuda.synchronize()

        def compose_host_v():
            compose_host()
            ctx._check(lib.eth_kzg_amd_verify_blob_cell_proofs_many(ctx.handle, n, vp(t_blobs), vp(t_comm), vp(t_proofs), ver, stt))

        def compose_device_v():
            compose_device()
            ctx._check(lib.eth_kzg_amd_verify_blob_cell_proofs_many_device(ctx.handle, n, dp(d_blobs), dp(d_comm), dp(d_proofs), ver, stt, None))

        def new_host(flags=0):
            ctx._check(lib.eth_kzg_amd_blobs_to_data_columns(ctx.handle, n, vp(t_blobs), vp(t_comm), vp(t_proofs), flags, vp(out["new"][4]), vp(out["new"][5]),
                                                             ver, stt))

        def new_device(flags=0):
            ctx._check(lib.eth_kzg_amd_blobs_to_data_columns_device(ctx.handle, n, dp(d_blobs), dp(d_comm), dp(d_proofs), flags, dp(d_out["new"][0]),
                                                                    dp(d_out["new"][1]), ver, stt, None))
            torch.cuda.synchronize()

        calls = {"compose_host": compose_host, "new_host": new_host, "compose_device": compose_device, "new_device": new_device,
                 "compose_host_v": compose_host_v, "new_host_v": lambda: new_host(VERIFY), "compose_device_v": compose_device_v,
                 "new_device_v": lambda: new_device(VERIFY)}

        def checked(kind):
            for i in range(n):
                ver[i] = False
                stt[i] = 7
            t0 = time.perf_counter()
            calls[kind]()
            ms = (time.perf_counter() - t0) * 1e3
            assert not any(stt) and (not kind.endswith("_v") or all(ver)), (kind, n)
            return ms

        kinds = list(calls)
        for new, old in PAIRS:  # the same bytes, road against road, before anything is timed
            for k in (0, 1):
                out["new"][k][:] = 0
                d_out["new"][k].zero_()
            checked(old)
            checked(new)
            if "host" in new:
                assert all(np.array_equal(out["new"][k], out["compose"][k]) for k in (0, 1)), (new, n)
            else:
                assert all(torch.equal(d_out["new"][k], d_out["compose"][k]) for k in (0, 1)), (new, n)
        for _ in range(3):
            for kind in kinds:
                checked(kind)
        samples = {k: [] for k in kinds}
        for i in range(a.rounds):
            for kind in kinds[i % len(kinds):] + kinds[:i % len(kinds)]:
                samples[kind].append(checked(kind))
        row = {"blobs": n, "kinds": {k: summary(v) for k, v in samples.items()}}
        k = row["kinds"]
        for new, old in PAIRS:
            row["%s_over_%s" % (old, new)] = k[old]["median_ms"] / k[new]["median_ms"]
            row["%s_slower_beyond_compose_spread" % new] = bool(k[new]["median_ms"] - k[old]["median_ms"] > k[old]["p90_ms"] - k[old]["p10_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d_proofs
    ctx.close()
    doc = {"what": "a block's data columns from blobs with their 128 cell proofs in hand, milliseconds per call: eth_kzg_amd_blobs_to_data_columns / "
                   "_device (flags = 0, and *_v with ETH_KZG_AMD_COLUMNS_VERIFY_PROOFS) against the composition a caller has without it -- "
                   "compute_data_columns with the cells alone plus a transposition of the proofs, and for *_v verify_blob_cell_proofs_many on "
                   "top; the composed calls run on this build's library, which does not change them; interleaved rounds in one process, default tables",
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "host_threads": os.environ.get("ETH_KZG_AMD_HOST_THREADS", "default"),
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
