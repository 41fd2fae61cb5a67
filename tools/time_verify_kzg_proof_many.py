"""Many verify_kzg_proof items per call against loops of the single call: the parent commit's, this build's, and the two new forms;
one process, one GPU.

    python tools/time_verify_kzg_proof_many.py --parent-lib PATH [--shapes 1,64,1024,16384,65536,16384:one,16384:1pc] [--rounds 25]
                                               [--out profiles/verify_kzg_proof_many.json]
    ETH_KZG_AMD_TRACE=1 python tools/time_verify_kzg_proof_many.py --laps [--shapes 16384]

A shape is N (all items valid), N:one (one wrong item in the middle) or N:1pc (1 % wrong items, scattered by a seed).  Items are valid
openings of 64 random blobs at one random point each, repeated to N; a wrong item has y + 1.  Per shape, on default tables, after three
warm-up calls of every kind, --rounds interleaved rounds; a round times every kind once, the order rotating from round to round; host
clock around each call (all are synchronous: they return verdicts).  Kinds:
    parent_loop   N calls of eth_kzg_verify_kzg_proof of --parent-lib (a libc_eth_kzg.so built from the parent commit, loaded next to
                  this build's, with a context of its own): the baseline.  N = 1 and 64 only.
    loop          the same on this build (N = 1 and 64 only): the single call is not to change
    many          eth_kzg_amd_verify_kzg_proof_many, pointer tables marshalled once
    many_device   eth_kzg_amd_verify_kzg_proof_many_device, flat arrays resident in HBM
Reported per kind: median, minimum, 10th and 90th percentile in milliseconds.  EVERY timed call's verdicts are checked against the
construction.  Conditions evaluated and written next to the figures: `loop` within the parent's p90 - p10 of the parent's median; at
N = 64 `many` faster than `parent_loop`.  Derived: the smallest all-valid N from which `many` beats the loop (the parent's per-item time
at 64 stands for larger N, labelled as that), items/s at the largest all-valid shape, what the wrong items cost against the all-valid
call.  --laps: no timing; with ETH_KZG_AMD_TRACE=1 in the environment the library prints the laps of one call of many / many_device per
shape on stderr, behind a line that names the call."""
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
N_BLOBS = 64
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
KINDS = ["parent_loop", "loop", "many", "many_device"]
LOOP_MAX = 64


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
    """the parent commit's product library, loaded next to this build's: its own context, its eth_kzg_verify_kzg_proof"""

    def __init__(self, path, kzg):
        self.lib = C.CDLL(os.path.abspath(path))
        P = C.c_void_p
        self.lib.eth_kzg_amd_das_context_new_on_device.restype = P
        self.lib.eth_kzg_amd_das_context_new_on_device.argtypes = [C.c_bool, C.c_int]
        self.lib.eth_kzg_amd_tables_ready.argtypes = [P, C.c_int]
        self.lib.eth_kzg_das_context_free.argtypes = [P]
        self.lib.eth_kzg_verify_kzg_proof.restype = kzg.CResult
        self.lib.eth_kzg_verify_kzg_proof.argtypes = [P, P, P, P, P, P]
        assert os.path.realpath(path) != os.path.realpath(kzg.load_library()._name), "--parent-lib is the library under test itself"
        self.ctx = C.c_void_p(self.lib.eth_kzg_amd_das_context_new_on_device(True, 0))
        while self.lib.eth_kzg_amd_tables_ready(self.ctx, 1000) == 0:
            pass

    def close(self):
        self.lib.eth_kzg_das_context_free(self.ctx)


def parse_shape(s):
    n, _, how = s.partition(":")
    assert how in ("", "one", "1pc"), s
    return int(n), how or "valid"


def wrong_places(n, how):
    if how == "one":
        return [n // 2]
    if how == "1pc":
        return sorted(random.Random("verify-kzg-proof-many:%d" % n).sample(range(n), max(1, n // 100)))
    return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1,64,1024,16384,65536,16384:one,16384:1pc")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--laps", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_kzg_proof_many.json"))
    a = ap.parse_args()
    shapes = [parse_shape(s) for s in a.shapes.split(",")]
    assert a.laps or a.parent_lib, "--parent-lib: the baseline is the parent commit's library"
    assert a.laps or a.rounds >= 25, "at least 25 interleaved rounds per shape"

    import torch
    torch.cuda.init()
    kzg = importlib.import_module("rust-eth-kzg_amd")
    lib = kzg.load_library()
    ctx = kzg.DASContext(use_precomp=True)
    parent = None if a.laps else ParentLibrary(a.parent_lib, kzg)
    blobs = random_blobs(N_BLOBS, 4844)
    bl = [blobs[b].tobytes() for b in range(N_BLOBS)]
    rng = random.Random("verify-kzg-proof-many:z")
    zs = [rng.randrange(R).to_bytes(32, "big") for _ in range(N_BLOBS)]
    st, proofs, ys = ctx.compute_kzg_proof_batch(bl, zs)
    assert st == [0] * N_BLOBS
    _, comms = ctx.blob_to_kzg_commitment_batch(bl)
    good = [(comms[b], zs[b], ys[b], proofs[b]) for b in range(N_BLOBS)]
    bad = [(c, z, ((int.from_bytes(y, "big") + 1) % R).to_bytes(32, "big"), p) for c, z, y, p in good]
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rows = []
    for n, how in shapes:
        wrong = set(wrong_places(n, how))
        items = [(bad if i in wrong else good)[i % N_BLOBS] for i in range(n)]
        want = [i not in wrong for i in range(n)]
        tabs = [kzg._flat_ptrs([it[k] for it in items], (48, 32, 32, 48)[k]) for k in range(4)]
        dev = [torch.from_numpy(t[1].copy()).cuda() for t in tabs]
        torch.cuda.synchronize()
        ptrs = [C.c_void_p(d.data_ptr()) for d in dev]
        ver, stt, one = (C.c_bool * n)(), (C.c_int32 * n)(), C.c_bool(False)
        bufs = [[C.create_string_buffer(f, len(f)) for f in it] for it in items[:LOOP_MAX]]

        def loop(fn, handle):
            for i in range(n):
                res = fn(handle, bufs[i][0], bufs[i][1], bufs[i][2], bufs[i][3], C.byref(one))
                assert res.status == 0
                ver[i] = one.value

        calls = {"many": lambda: ctx._check(lib.eth_kzg_amd_verify_kzg_proof_many(ctx.handle, n, *[vp(t[0]) for t in tabs], ver, stt)),
                 "many_device": lambda: ctx._check(lib.eth_kzg_amd_verify_kzg_proof_many_device(ctx.handle, n, *ptrs, ver, stt, None))}
        if n <= LOOP_MAX:
            lib.eth_kzg_verify_kzg_proof.argtypes = [C.c_void_p] * 6
            calls["loop"] = lambda: loop(lib.eth_kzg_verify_kzg_proof, ctx.handle)
            if parent:
                calls["parent_loop"] = lambda: loop(parent.lib.eth_kzg_verify_kzg_proof, parent.ctx)

        def checked(kind):
            for i in range(n):
                ver[i] = False
                stt[i] = 0
            t0 = time.perf_counter()
            calls[kind]()
            ms = (time.perf_counter() - t0) * 1e3
            assert list(ver) == want and not any(stt), (kind, n, how)
            return ms

        kinds = [k for k in KINDS if k in calls]
        for _ in range(3):
            for kind in kinds:
                checked(kind)
        if a.laps:
            for kind in ("many", "many_device"):
                print("[laps] %d %s %s" % (n, how, kind), file=sys.stderr, flush=True)
                checked(kind)
            continue
        samples = {k: [] for k in kinds}
        for i in range(a.rounds):
            for kind in kinds[i % len(kinds):] + kinds[:i % len(kinds)]:
                samples[kind].append(checked(kind))
        row = {"items": n, "wrong": how, "wrong_items": len(wrong), "kinds": {k: summary(v) for k, v in samples.items()}}
        if "parent_loop" in row["kinds"]:
            p, lp, m = row["kinds"]["parent_loop"], row["kinds"]["loop"], row["kinds"]["many"]
            row["loop_within_parent_spread"] = bool(abs(lp["median_ms"] - p["median_ms"]) <= p["p90_ms"] - p["p10_ms"])
            row["many_faster_than_parent_loop"] = bool(m["median_ms"] < p["median_ms"])
            row["parent_loop_over_many"] = p["median_ms"] / m["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del dev
    if parent:
        parent.close()
    ctx.close()
    if a.laps:
        return
    derived = {}
    valid = {r["items"]: r for r in rows if r["wrong"] == "valid"}
    if 64 in valid and "parent_loop" in valid[64]["kinds"]:
        per_item = valid[64]["kinds"]["parent_loop"]["median_ms"] / 64
        derived["parent_loop_ms_per_item_at_64"] = per_item
        derived["condition_many_faster_than_parent_loop_at_64"] = valid[64]["many_faster_than_parent_loop"]
        beats = [n for n in sorted(valid) if valid[n]["kinds"]["many"]["median_ms"] <
                 (valid[n]["kinds"]["parent_loop"]["median_ms"] if "parent_loop" in valid[n]["kinds"] else per_item * n)]
        derived["smallest_measured_n_where_many_beats_the_loop"] = beats[0] if beats else None
        derived["loop_figures_above_64_are"] = "the parent's per-item time at 64 times n"
    if valid:
        top = max(valid)
        for k in ("many", "many_device"):
            derived["items_per_s_at_%d_%s" % (top, k)] = top / (valid[top]["kinds"][k]["median_ms"] / 1e3)
    for r in rows:
        if r["wrong"] != "valid" and r["items"] in valid:
            for k in ("many", "many_device"):
                derived["%s_%d_%s_over_all_valid" % (k, r["items"], r["wrong"])] = r["kinds"][k]["median_ms"] / valid[r["items"]]["kinds"][k]["median_ms"]
    doc = {"what": "verify_kzg_proof for many items, milliseconds per call: loops of the parent commit's and of this build's single call, "
                   "eth_kzg_amd_verify_kzg_proof_many, _many_device; interleaved rounds in one process, default tables",
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "host_threads": os.environ.get("ETH_KZG_AMD_HOST_THREADS", "default"),
           "rows": rows, "derived": derived}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
