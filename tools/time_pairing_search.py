"""The search of the "many" verifications for their wrong entries with its pairings on the GPU (k_pairing_check), measured; one process,
one GPU, default tables.

    python tools/time_pairing_search.py --parent-lib PATH [--rounds 25] [--sizes 16,32,...,4096] [--out profiles/pairing_search.json]

(a) Crossover.  The hook eth_kzg_amd_test_pairing_check_many (the hooks library) at n = 16 .. 4096 pairs, both pairs of keys, half of the
    pairs valid: the GPU route (launch, verdict bytes down, wait) against the host threads' checks of the same pairs (parallel_for over
    check_pair at the context's thread count), nanoseconds from the library's own clock (eth_kzg_amd_test_search_stats), --hook-rounds
    calls each, medians; both sides' verdicts checked against the construction on every call.  The knob's value: the smallest measured n
    from which the GPU route is not slower at that n or at any larger measured n, for both keys (0 if there is none).  The first
    launch of the process is reported apart (it sets up the kernel's scratch memory).
(b) Calls.  eth_kzg_amd_verify_kzg_proof_many at 16384 items with 0, 1, 1 %, 25 % and 100 % wrong and
    eth_kzg_amd_verify_cell_kzg_proof_batch_many at 1024 problems of 128 cells with 0, 1 and 100 % wrong, this build (context made with
    ETH_KZG_AMD_GPU_PAIRING_MIN = the value (a) chose) against --parent-lib (a libc_eth_kzg.so built from the parent commit, loaded next
    to this build's, a context of its own), after three warm-up calls of each, --rounds interleaved rounds with the order alternating;
    host clock around each call; EVERY timed call's verdicts are checked against the construction.  Per kind: median, minimum, p10, p90.
    Conditions written next to the figures: at 25 % and 100 % wrong this build's median is below the parent's by more than the two
    p10-p90 spreads added; at 0 and 1 wrong it lies within the parent's p10-p90."""
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
os.environ.setdefault("ETH_KZG_AMD_LIB", os.path.join(ROOT, "rust-eth-kzg_amd", "libc_eth_kzg_hooks.so"))
SETUP = os.path.join(ROOT, "rust-eth-kzg_amd", "data", "trusted_setup_4096.bin")
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N_BLOBS = 64


def summary(ms):
    s = sorted(ms)
    pick = lambda q: s[min(len(s) - 1, int(q * len(s)))]  # noqa: E731
    return {"median_ms": statistics.median(s), "min_ms": s[0], "p10_ms": pick(0.10), "p90_ms": pick(0.90), "calls": len(s)}


def random_blobs(n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, 4096, 32), dtype=np.uint8)
    a[:, :, 0] &= 0x3F  # < 2^254 < r: canonical field elements
    return a.reshape(n, 131072)


class ParentLibrary:
    """the parent commit's product library, loaded next to this build's: its own context, its two many-verifications"""

    def __init__(self, path, kzg):
        self.lib = C.CDLL(os.path.abspath(path))
        P = C.c_void_p
        self.lib.eth_kzg_amd_das_context_new_on_device.restype = P
        self.lib.eth_kzg_amd_das_context_new_on_device.argtypes = [C.c_bool, C.c_int]
        self.lib.eth_kzg_amd_tables_ready.argtypes = [P, C.c_int]
        self.lib.eth_kzg_das_context_free.argtypes = [P]
        for name, count in (("eth_kzg_amd_verify_kzg_proof_many", 8), ("eth_kzg_amd_verify_cell_kzg_proof_batch_many", 12)):
            getattr(self.lib, name).restype = kzg.CResult
            getattr(self.lib, name).argtypes = [P, C.c_uint64] + [P] * (count - 2)
        assert not hasattr(self.lib, "eth_kzg_amd_test_search_stats"), "--parent-lib is the product library of the parent commit"
        self.ctx = C.c_void_p(self.lib.eth_kzg_amd_das_context_new_on_device(True, 0))
        while self.lib.eth_kzg_amd_tables_ready(self.ctx, 1000) == 0:
            pass

    def close(self):
        self.lib.eth_kzg_das_context_free(self.ctx)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
def crossover(kzg, ctx, sizes, rounds):
    lib = kzg.load_library()
    with open(SETUP, "rb") as f:
        srs = f.read()
    S = lambda i: srs[16 + 48 * i:16 + 48 * i + 48]  # noqa: E731
    stats = (C.c_uint64 * 4)()
    rows, first_ms = [], None
    for key, k in ((0, 64), (1, 1)):
        for n in sizes:
            # (S_i, S_(i+k)) passes; (S_i, S_(i+k+1)) does not
            pairs = b"".join(S(e % 3000) + S(e % 3000 + k + (e & 1)) for e in range(n))
            want = [1 - (e & 1) for e in range(n)]
            gpu, host = (C.c_int8 * n)(), (C.c_int8 * n)()
            g_ms, h_ms = [], []
            for r in range(rounds + 1):
                assert lib.eth_kzg_amd_test_pairing_check_many(ctx.handle, key, n, pairs, 0, gpu, host, None, None) == 0
                assert list(gpu) == want and list(host) == want, (key, n)
                assert lib.eth_kzg_amd_test_search_stats(ctx.handle, stats) == 0
                if first_ms is None:
                    first_ms = stats[2] / 1e6
                if r:  # (the first call of a size warms up)
                    g_ms.append(stats[2] / 1e6)
                    h_ms.append(stats[3] / 1e6)
            row = {"key": key, "pairs": n, "gpu": summary(g_ms), "host_threads": summary(h_ms)}
            row["gpu_not_slower"] = bool(row["gpu"]["median_ms"] <= row["host_threads"]["median_ms"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    chosen = 0
    for n in sorted(sizes, reverse=True):
        if all(r["gpu_not_slower"] for r in rows if r["pairs"] >= n):
            chosen = n
        else:
            break
    return rows, chosen, first_ms


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------
def wrong_places(n, how):
    if how == "0":
        return []
    if how == "1":
        return [n // 2]
    share = {"1pc": 100, "25pc": 4, "100pc": 1}[how]
    return list(range(n)) if share == 1 else sorted(random.Random("pairing-search:%d:%s" % (n, how)).sample(range(n), n // share))


def time_kinds(calls, rounds, check):
    kinds = list(calls)
    for _ in range(3):
        for k in kinds:
            check(k, calls[k])
    samples = {k: [] for k in kinds}
    for i in range(rounds):
        for k in (kinds if i % 2 == 0 else kinds[::-1]):
            samples[k].append(check(k, calls[k]))
    return {k: summary(v) for k, v in samples.items()}


def conditions(row):
    p, m, how = row["kinds"]["parent"], row["kinds"]["this_build"], row["wrong"]
    if how in ("25pc", "100pc"):
        row["condition"] = "median below the parent's by more than the two p10-p90 spreads added"
        row["condition_met"] = bool(p["median_ms"] - m["median_ms"] > (p["p90_ms"] - p["p10_ms"]) + (m["p90_ms"] - m["p10_ms"]))
    elif how in ("0", "1"):
        row["condition"] = "median within the parent's p10-p90"
        row["condition_met"] = bool(p["p10_ms"] <= m["median_ms"] <= p["p90_ms"])
    row["parent_over_this_build"] = p["median_ms"] / m["median_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,32,64,128,256,512,1024,2048,4096")
    ap.add_argument("--hook-rounds", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--points", default="0,1,1pc,25pc,100pc")
    ap.add_argument("--cells", default="0,1,100pc")
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing_search.json"))
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]

    import torch
    torch.cuda.init()
    kzg = importlib.import_module("rust-eth-kzg_amd")
    lib = kzg.load_library()
    os.environ.pop("ETH_KZG_AMD_GPU_PAIRING_MIN", None)
    ctx0 = kzg.DASContext(use_precomp=True)
    hook_rows, chosen, first_ms = crossover(kzg, ctx0, sizes, a.hook_rounds)
    print(json.dumps({"chosen_gpu_pairing_min": chosen, "first_launch_ms": first_ms}), flush=True)
    ctx0.close()
    os.environ["ETH_KZG_AMD_GPU_PAIRING_MIN"] = str(chosen)
    ctx = kzg.DASContext(use_precomp=True)
    os.environ.pop("ETH_KZG_AMD_GPU_PAIRING_MIN", None)
    parent = ParentLibrary(a.parent_lib, kzg)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rows = []

    # ---- verify_kzg_proof_many, 16384 items
    blobs = random_blobs(N_BLOBS, 4844)
    bl = [blobs[b].tobytes() for b in range(N_BLOBS)]
    rng = random.Random("pairing-search:z")
    zs = [rng.randrange(R).to_bytes(32, "big") for _ in range(N_BLOBS)]
    st, proofs, ys = ctx.compute_kzg_proof_batch(bl, zs)
    assert st == [0] * N_BLOBS
    _, comms = ctx.blob_to_kzg_commitment_batch(bl)
    good = [(comms[b], zs[b], ys[b], proofs[b]) for b in range(N_BLOBS)]
    bad = [(c, z, ((int.from_bytes(y, "big") + 1) % R).to_bytes(32, "big"), p) for c, z, y, p in good]
    n = 16384
    for how in [h for h in a.points.split(",") if h]:
        wrong = set(wrong_places(n, how))
        items = [(bad if i in wrong else good)[i % N_BLOBS] for i in range(n)]
        want = [i not in wrong for i in range(n)]
        tabs = [kzg._flat_ptrs([it[k] for it in items], (48, 32, 32, 48)[k]) for k in range(4)]
        ver, stt = (C.c_bool * n)(), (C.c_int32 * n)()
        calls = {"this_build": lambda: ctx._check(lib.eth_kzg_amd_verify_kzg_proof_many(ctx.handle, n, *[vp(t[0]) for t in tabs], ver, stt)),
                 "parent": lambda: ctx._check(parent.lib.eth_kzg_amd_verify_kzg_proof_many(parent.ctx, n, *[vp(t[0]) for t in tabs], ver, stt))}

        def check(kind, call):
            C.memset(ver, 0, n)
            t0 = time.perf_counter()
            call()
            ms = (time.perf_counter() - t0) * 1e3
            assert list(ver) == want and not any(stt), (kind, how)
            return ms

        row = {"call": "verify_kzg_proof_many", "entries": n, "wrong": how, "wrong_entries": len(wrong), "kinds": time_kinds(calls, a.rounds, check)}
        conditions(row)
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- verify_cell_kzg_proof_batch_many, 1024 problems of 128 cells
    st, cells, cproofs = ctx.compute_cells_and_kzg_proofs_batch(bl[:2])
    assert st == [0, 0]
    nb = 1024
    for how in [h for h in a.cells.split(",") if h]:
        wrong = set(wrong_places(nb, how))
        problems = []
        for b in range(nb):
            pr = list(cproofs[b % 2])
            if b in wrong:
                pr[5], pr[77] = pr[77], pr[5]
            problems.append(([comms[b % 2]] * 128, list(range(128)), cells[b % 2], pr))
        want = [b not in wrong for b in range(nb)]
        _, lens, tabs, keep = ctx._marshal_many(problems)
        del problems
        ver, stt = (C.c_bool * nb)(), (C.c_int32 * nb)()
        args = [x for k in range(4) for x in (vp(lens[k]), vp(tabs[k]))]
        calls = {"this_build": lambda: ctx._check(lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many(ctx.handle, nb, *args, ver, stt)),
                 "parent": lambda: ctx._check(parent.lib.eth_kzg_amd_verify_cell_kzg_proof_batch_many(parent.ctx, nb, *args, ver, stt))}

        def check(kind, call):
            C.memset(ver, 0, nb)
            t0 = time.perf_counter()
            call()
            ms = (time.perf_counter() - t0) * 1e3
            assert list(ver) == want and not any(stt), (kind, how)
            return ms

        row = {"call": "verify_cell_kzg_proof_batch_many", "entries": nb, "cells_per_problem": 128, "wrong": how, "wrong_entries": len(wrong),
               "kinds": time_kinds(calls, a.rounds, check)}
        conditions(row)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del keep
    parent.close()
    ctx.close()
    doc = {"what": "k_pairing_check against the host threads' pairing checks (hook, milliseconds per batch of pairs), and the many-verifications "
                   "with wrong entries against the parent commit's library (milliseconds per call); one process, default tables",
           "device": torch.cuda.get_device_name(0), "host_threads": os.environ.get("ETH_KZG_AMD_HOST_THREADS", "default"),
           "hook_rounds": a.hook_rounds, "rounds": a.rounds, "first_launch_ms": first_ms, "crossover": hook_rows, "chosen_gpu_pairing_min": chosen,
           "calls": rows, "all_conditions_met": all(r.get("condition_met", True) for r in rows)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
