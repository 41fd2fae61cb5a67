"""Many verify_blob_kzg_proof items per call, a verdict each, against its two baselines; one process, one GPU.

    python tools/time_verify_blob_kzg_proof_many.py --parent-lib PATH [--shapes 1,6,64,512] [--rounds 25]
                                                    [--out profiles/verify_blob_kzg_proof_many.json]
    ETH_KZG_AMD_TRACE=1 python tools/time_verify_blob_kzg_proof_many.py --laps [--shapes 64]

Items are N valid (blob, commitment, proof) triples of N distinct random blobs (proofs from eth_kzg_amd_compute_blob_kzg_proof_batch); the
host form's pointer tables are marshalled once, the device form's arrays are resident in HBM.  Per shape, on default tables, after three
warm-up calls of every kind, --rounds interleaved rounds; a round times every kind once, the order rotating from round to round; host
clock around each call (all are synchronous: they return verdicts).  Kinds:
    parent_loop    N calls of eth_kzg_verify_blob_kzg_proof of --parent-lib (a libc_eth_kzg.so built from the parent commit, loaded next
                   to this build's, with a context of its own): what a client does today to find the wrong blob of a failed batch
    loop           the same on this build: the single call is not to change
    batch          ONE eth_kzg_verify_blob_kzg_proof_batch call of this build: one verdict for all N
    batch_device   ONE eth_kzg_amd_verify_blob_kzg_proof_batch_device call: the same on resident arrays
    many           eth_kzg_amd_verify_blob_kzg_proof_many: a verdict each
    many_device    eth_kzg_amd_verify_blob_kzg_proof_many_device
Reported per kind: median, minimum, 10th and 90th percentile in milliseconds.  EVERY timed call's verdicts are checked.  Nothing is
gated: the ratios are written next to the figures (parent_loop over many, many over batch, many_device over batch_device), and where the
new call loses it says so.  A second pass per shape plants ONE wrong proof in the middle and times `many` / `many_device` again (the
search).  --laps: no timing; with ETH_KZG_AMD_TRACE=1 the library prints the laps of one call of many / many_device per shape on stderr."""
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
KINDS = ["parent_loop", "loop", "batch", "batch_device", "many", "many_device"]
BLOB = 131072


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
    """the parent commit's product library, loaded next to this build's: its own context, its eth_kzg_verify_blob_kzg_proof"""

    def __init__(self, path, kzg):
        self.lib = C.CDLL(os.path.abspath(path))
        P = C.c_void_p
        self.lib.eth_kzg_amd_das_context_new_on_device.restype = P
        self.lib.eth_kzg_amd_das_context_new_on_device.argtypes = [C.c_bool, C.c_int]
        self.lib.eth_kzg_amd_tables_ready.argtypes = [P, C.c_int]
        self.lib.eth_kzg_das_context_free.argtypes = [P]
        self.lib.eth_kzg_verify_blob_kzg_proof.restype = kzg.CResult
        self.lib.eth_kzg_verify_blob_kzg_proof.argtypes = [P, P, P, P, P]
        assert os.path.realpath(path) != os.path.realpath(kzg.load_library()._name), "--parent-lib is the library under test itself"
        self.ctx = C.c_void_p(self.lib.eth_kzg_amd_das_context_new_on_device(True, 0))
        while self.lib.eth_kzg_amd_tables_ready(self.ctx, 1000) == 0:
            pass

    def close(self):
        self.lib.eth_kzg_das_context_free(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1,6,64,512")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--laps", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_blob_kzg_proof_many.json"))
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
    blobs = random_blobs(top, 4844)
    bl = [blobs[b].tobytes() for b in range(top)]
    _, comms = ctx.blob_to_kzg_commitment_batch(bl)
    st, proofs = ctx.compute_blob_kzg_proof_batch(bl, comms)
    assert st == [0] * top
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    lib.eth_kzg_verify_blob_kzg_proof.argtypes = [C.c_void_p] * 5
    lib.eth_kzg_verify_blob_kzg_proof_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    rows = []
    for n in shapes:
        for wrong in ([], [n // 2]):
            if wrong and n < 2:
                continue
            pr = list(proofs[:n])
            for i in wrong:
                pr[i] = proofs[(i + 1) % n]
            want = [i not in wrong for i in range(n)]
            tabs = [kzg._flat_ptrs(bl[:n], BLOB), kzg._flat_ptrs(comms[:n], 48), kzg._flat_ptrs(pr, 48)]
            dev = [torch.from_numpy(t[1].copy()).cuda() for t in tabs]
            torch.cuda.synchronize()
            ptrs = [C.c_void_p(d.data_ptr()) for d in dev]
            ver, stt, one = (C.c_bool * n)(), (C.c_int32 * n)(), C.c_bool(False)

            def loop(fn, handle):
                for i in range(n):
                    res = fn(handle, C.c_void_p(int(tabs[0][0][i])), C.c_void_p(int(tabs[1][0][i])), C.c_void_p(int(tabs[2][0][i])), C.byref(one))
                    assert res.status == 0
                    ver[i] = one.value

            def batch():
                ctx._check(lib.eth_kzg_verify_blob_kzg_proof_batch(ctx.handle, n, vp(tabs[0][0]), n, vp(tabs[1][0]), n, vp(tabs[2][0]), C.byref(one)))
                for i in range(n):
                    ver[i] = one.value

            def batch_device():
                ctx._check(lib.eth_kzg_amd_verify_blob_kzg_proof_batch_device(ctx.handle, n, *ptrs, C.byref(one), None))
                for i in range(n):
                    ver[i] = one.value

            calls = {"many": lambda: ctx._check(lib.eth_kzg_amd_verify_blob_kzg_proof_many(ctx.handle, n, *[vp(t[0]) for t in tabs], ver, stt)),
                     "many_device": lambda: ctx._check(lib.eth_kzg_amd_verify_blob_kzg_proof_many_device(ctx.handle, n, *ptrs, ver, stt, None))}
            if not wrong:
                calls.update({"loop": lambda: loop(lib.eth_kzg_verify_blob_kzg_proof, ctx.handle), "batch": batch, "batch_device": batch_device})
                if parent:
                    calls["parent_loop"] = lambda: loop(parent.lib.eth_kzg_verify_blob_kzg_proof, parent.ctx)

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
                for kind in ("many", "many_device"):
                    print("[laps] %d wrong=%s %s" % (n, wrong, kind), file=sys.stderr, flush=True)
                    checked(kind)
                continue
            samples = {k: [] for k in kinds}
            for i in range(a.rounds):
                for kind in kinds[i % len(kinds):] + kinds[:i % len(kinds)]:
                    samples[kind].append(checked(kind))
            row = {"items": n, "wrong_items": len(wrong), "kinds": {k: summary(v) for k, v in samples.items()}}
            k = row["kinds"]
            if "parent_loop" in k:
                row["parent_loop_over_many"] = k["parent_loop"]["median_ms"] / k["many"]["median_ms"]
                row["parent_loop_over_many_device"] = k["parent_loop"]["median_ms"] / k["many_device"]["median_ms"]
                row["loop_within_parent_spread"] = bool(abs(k["loop"]["median_ms"] - k["parent_loop"]["median_ms"]) <= k["parent_loop"]["p90_ms"] - k["parent_loop"]["p10_ms"])
            if "batch" in k:
                row["many_over_batch"] = k["many"]["median_ms"] / k["batch"]["median_ms"]
                row["many_device_over_batch_device"] = k["many_device"]["median_ms"] / k["batch_device"]["median_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            del dev
    if parent:
        parent.close()
    ctx.close()
    if a.laps:
        return
    doc = {"what": "verify_blob_kzg_proof for many items, milliseconds per call: loops of the parent commit's and of this build's single call, "
                   "one batch call (one verdict), eth_kzg_amd_verify_blob_kzg_proof_many / _many_device (a verdict each); interleaved "
                   "rounds in one process, default tables; wrong_items = 1: the search for one planted wrong proof",
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "host_threads": os.environ.get("ETH_KZG_AMD_HOST_THREADS", "default"),
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
