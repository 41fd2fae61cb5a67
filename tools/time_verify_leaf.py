"""verify_cell_kzg_proof_batch with and without the leaf-hashed challenge (ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT), same process, same context.

    python tools/time_verify_leaf.py [--ns 128,1024,8192] [--runs 25] [--out profiles/r7_verify_leaf_transcript.json]

Per n (cells of 64 distinct blobs, n / 64 cells of each, so the batch has 64 commitment rows) and per form -- "host": the host-pointer
calls eth_kzg_verify_cell_kzg_proof_batch / eth_kzg_amd_verify_cell_kzg_proof_batch_ex on pointer tables marshalled once; "device": the
device-resident calls on flat arrays in HBM -- three warm-up calls of each kind, then --runs PAIRS of timed calls, the flagged and the
unflagged call alternating (and the order inside a pair alternating), host clock around each call (both calls are synchronous: they
return a verdict).  Reported: median, minimum, 10th and 90th percentile of each kind in milliseconds, and unflagged / flagged of the
medians.  Every timed call must verify.  With ETH_KZG_AMD_TRACE=1 in the environment the library prints the laps of every call on
stderr ("leaf hashes (GPU) + root (host)" against "sha256 transcript (host)"); time without it."""
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


def random_blobs(n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, 4096, 32), dtype=np.uint8)
    a[:, :, 0] &= 0x3F  # < 2^254 < r: canonical field elements
    return a.reshape(n, 131072)


def summary(ms):
    s = sorted(ms)
    pick = lambda q: s[min(len(s) - 1, int(q * len(s)))]  # noqa: E731
    return {"median_ms": statistics.median(s), "min_ms": s[0], "p10_ms": pick(0.10), "p90_ms": pick(0.90), "calls": len(s)}


def interleaved(flagged, unflagged, runs):
    for _ in range(3):
        assert flagged() and unflagged()
    out = {"flagged": [], "unflagged": []}
    for i in range(runs):
        for kind in (("flagged", "unflagged") if i % 2 == 0 else ("unflagged", "flagged")):
            fn = flagged if kind == "flagged" else unflagged
            t0 = time.perf_counter()
            ok = fn()
            out[kind].append((time.perf_counter() - t0) * 1e3)
            assert ok, kind
    row = {k: summary(v) for k, v in out.items()}
    row["unflagged_over_flagged"] = row["unflagged"]["median_ms"] / row["flagged"]["median_ms"]
    # the difference of the medians against the wider of the two p10 .. p90 spreads
    spread = max(row[k]["p90_ms"] - row[k]["p10_ms"] for k in ("flagged", "unflagged"))
    row["median_difference_ms"] = row["unflagged"]["median_ms"] - row["flagged"]["median_ms"]
    row["wider_spread_ms"] = spread
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="128,1024,8192")
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7_verify_leaf_transcript.json"))
    a = ap.parse_args()
    ns = [int(x) for x in a.ns.split(",")]
    assert a.runs >= 20 and all(n % N_BLOBS == 0 and n <= N_BLOBS * 128 for n in ns)

    import torch
    torch.cuda.init()
    kzg = importlib.import_module("rust-eth-kzg_amd")
    lib = kzg.load_library()
    ctx = kzg.DASContext(use_precomp=True)
    blobs = random_blobs(N_BLOBS, 7594)
    bl = [blobs[b].tobytes() for b in range(N_BLOBS)]
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(bl)
    assert st == [0] * N_BLOBS
    _, comms = ctx.blob_to_kzg_commitment_batch(bl)

    rows = []
    for n in ns:
        per = n // N_BLOBS
        entries = [(b, c) for c in range(per) for b in range(N_BLOBS)]  # interleaved: neighbours belong to different rows
        comm, idx = [comms[b] for b, _ in entries], [c for _, c in entries]
        cl, pr = [cells[b][c] for b, c in entries], [proofs[b][c] for b, c in entries]
        # host form: the C ABI's pointer tables, marshalled once
        ca, k1 = kzg._flat_ptrs(comm, 48)
        la, k2 = kzg._flat_ptrs(cl, 2048)
        pa, k3 = kzg._flat_ptrs(pr, 48)
        ia = np.array(idx, dtype=np.uint64)

        def host(flags):
            ok = C.c_bool(False)
            if flags:
                res = lib.eth_kzg_amd_verify_cell_kzg_proof_batch_ex(ctx.handle, n, kzg._vp(ca), n, kzg._vp(ia), n, kzg._vp(la), n, kzg._vp(pa), flags, C.byref(ok))
            else:
                res = lib.eth_kzg_verify_cell_kzg_proof_batch(ctx.handle, n, kzg._vp(ca), n, kzg._vp(ia), n, kzg._vp(la), n, kzg._vp(pa), C.byref(ok))
            ctx._check(res)
            return bool(ok.value)

        dev = lambda raw: torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()  # noqa: E731
        d_c, d_l, d_p = dev(b"".join(comm)), dev(b"".join(cl)), dev(b"".join(pr))
        d_i = torch.from_numpy(np.array(idx, dtype=np.int64)).cuda()
        torch.cuda.synchronize()
        ptrs = (n, d_c.data_ptr(), d_i.data_ptr(), d_l.data_ptr(), d_p.data_ptr())
        row = {"n": n,
               "host": interleaved(lambda: host(kzg.VERIFY_LEAF_TRANSCRIPT), lambda: host(0), a.runs),
               "device": interleaved(lambda: ctx.verify_cell_kzg_proof_batch_device(*ptrs, leaf_transcript=True),
                                     lambda: ctx.verify_cell_kzg_proof_batch_device(*ptrs), a.runs)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del k1, k2, k3
    ctx.close()
    doc = {"what": "verify_cell_kzg_proof_batch, n cells of 64 distinct blobs: the leaf-hashed challenge (flagged) against the reference's transcript "
                   "(unflagged), interleaved in one process on one context; host clock around synchronous calls, milliseconds",
           "timed_pairs": a.runs, "warm_up_calls_of_each_kind": 3, "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
