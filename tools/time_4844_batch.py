"""EIP-4844 blob proofs for n blobs: n single calls against the host batch form and the device-resident form.

    python tools/time_4844_batch.py [--ns 1,6,64,2048] [--runs 10] [--parent-lib PATH] [--out profiles/eip4844_batch_timings.json]

Per n (warm-up first, then the median of --runs runs, all in one process on one GPU):
  single_calls_ms   n calls of eth_kzg_compute_blob_kzg_proof, one after the other.  With --parent-lib (a libc_eth_kzg.so built from
                    the parent commit) they run in a child process on that library, in the same session; otherwise on the library in
                    use, whose single entry points are the same code.
  host_batch_ms     eth_kzg_amd_compute_blob_kzg_proof_batch on n host pointers (host clock; the call is synchronous)
  device_ms         eth_kzg_amd_compute_blob_kzg_proof_device on resident blobs, status = NULL, on a caller's stream: HIP events around it
  device_no_hash_ms eth_kzg_amd_compute_kzg_proof_device on the same blobs (the same opening without the challenge hash), HIP events
  hash_ms           the hash kernel on its own through its test hook (needs libc_eth_kzg_hooks.so; the hook uploads 32 bytes, launches
                    and synchronises: host clock around it)
The proofs of the three forms are compared before anything is timed.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
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


def median_ms(fn, runs):
    fn()  # warm-up
    fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def time_single_calls(ns, runs, nmax):
    kzg = importlib.import_module("rust-eth-kzg_amd")
    ctx = kzg.DASContext(use_precomp=True)
    blobs = random_blobs(nmax, 4844)
    bl = [blobs[b].tobytes() for b in range(nmax)]
    _, comms = ctx.blob_to_kzg_commitment_batch(bl)
    res = {}
    for n in ns:
        res[n] = median_ms(lambda: [ctx.compute_blob_kzg_proof(bl[b], comms[b]) for b in range(n)], runs if n < 1024 else max(3, runs // 3))
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1,6,64,2048")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--single-only", action="store_true", help="(child mode) print the single-call timings as JSON and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eip4844_batch_timings.json"))
    a = ap.parse_args()
    ns = [int(x) for x in a.ns.split(",")]
    nmax = max(ns)
    if a.single_only:
        print("SINGLE " + json.dumps(time_single_calls(ns, a.runs, nmax)))
        return

    import torch
    torch.cuda.init()
    kzg = importlib.import_module("rust-eth-kzg_amd")
    hooks = os.path.exists(kzg.HOOKS_LIB_PATH) and "ETH_KZG_AMD_LIB" not in os.environ
    if hooks:
        os.environ["ETH_KZG_AMD_LIB"] = kzg.HOOKS_LIB_PATH  # the product's objects + the hash kernel's hook
    lib = kzg.load_library()
    ctx = kzg.DASContext(use_precomp=True)
    blobs = random_blobs(nmax, 4844)
    bl = [blobs[b].tobytes() for b in range(nmax)]
    _, comms = ctx.blob_to_kzg_commitment_batch(bl)
    zs = [bytes([b & 0x3F]) + bytes(30) + bytes([b % 251 + 1]) for b in range(nmax)]
    d_blobs = torch.from_numpy(blobs.reshape(-1)).cuda()
    d_comms = torch.from_numpy(np.frombuffer(b"".join(comms), dtype=np.uint8).copy()).cuda()
    d_zs = torch.from_numpy(np.frombuffer(b"".join(zs), dtype=np.uint8).copy()).cuda()
    d_proofs = torch.zeros(nmax * 48, dtype=torch.uint8, device="cuda")
    d_ys = torch.zeros(nmax * 32, dtype=torch.uint8, device="cuda")
    d_dig = torch.zeros(nmax * 32, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    prefix = b"FSBLOBVERIFY_V1_" + (4096).to_bytes(16, "big")

    def events_ms(enqueue, runs):
        def once():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            enqueue()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)
        once()
        once()
        return statistics.median(once() for _ in range(runs))

    # results first: the three forms agree
    k = min(nmax, 70)
    st, want = ctx.compute_blob_kzg_proof_batch(bl[:k], comms[:k])
    assert st == [0] * k and want[:3] == [ctx.compute_blob_kzg_proof(bl[b], comms[b]) for b in range(3)]
    assert ctx.compute_blob_kzg_proof_device(k, d_blobs.data_ptr(), d_comms.data_ptr(), d_proofs.data_ptr()) == [0] * k
    assert d_proofs[:k * 48].cpu().numpy().tobytes() == b"".join(want)

    if a.parent_lib:
        env = dict(os.environ, ETH_KZG_AMD_LIB=os.path.abspath(a.parent_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--single-only", "--ns", a.ns, "--runs", str(a.runs)],
                             env=env, capture_output=True, text=True, check=True).stdout
        single = {int(k_): v for k_, v in json.loads([l for l in out.splitlines() if l.startswith("SINGLE ")][0][7:]).items()}
    else:
        single = None
    rows = []
    for n in ns:
        runs = a.runs if n < 1024 else max(3, a.runs // 3)
        row = {"n": n}
        row["single_calls_ms"] = single[n] if single else median_ms(lambda: [ctx.compute_blob_kzg_proof(bl[b], comms[b]) for b in range(n)], runs)
        prepared = (bl[:n], comms[:n])
        row["host_batch_ms"] = median_ms(lambda: ctx.compute_blob_kzg_proof_batch(*prepared), runs)
        row["device_ms"] = events_ms(lambda: ctx.compute_blob_kzg_proof_device(n, d_blobs.data_ptr(), d_comms.data_ptr(), d_proofs.data_ptr(),
                                                                               want_status=False, stream=stream.cuda_stream), runs)
        row["device_no_hash_ms"] = events_ms(lambda: ctx.compute_kzg_proof_device(n, d_blobs.data_ptr(), d_zs.data_ptr(), d_proofs.data_ptr(),
                                                                                  d_ys.data_ptr(), want_status=False, stream=stream.cuda_stream), runs)
        if hooks:
            row["hash_ms"] = median_ms(lambda: lib.eth_kzg_amd_test_sha256_many(ctx.handle, n, prefix, 32, d_blobs.data_ptr(), 131072, 131072,
                                                                                d_comms.data_ptr(), 48, 48, d_dig.data_ptr()), runs)
        row["single_over_host_batch"] = row["single_calls_ms"] / row["host_batch_ms"]
        row["single_over_device"] = row["single_calls_ms"] / row["device_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    doc = {"what": "compute_blob_kzg_proof for n blobs: n single calls, host batch form, device-resident form (milliseconds, medians)",
           "runs": a.runs, "single_calls_on": "parent library (child process)" if a.parent_lib else "library in use",
           "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
