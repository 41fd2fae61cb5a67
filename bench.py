#!/usr/bin/env python3
"""bench.py -- blobs/s of compute_cells_and_kzg_proofs on MI355X (BASELINE.json's metric).

    python bench.py --gpus N --steps K --warmup W        (N > 1: bench.py itself starts one rank per GPU, see _launch)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W
    python bench.py --gpus 2 --launcher-selftest          (CPU only: the launcher and the rendezvous, no GPU work)
    python bench.py ... --full                            (also every side figure and check, see below)
    python bench.py ... --dump-outputs DIR                (the last timed step's cells and proofs as DIR/<name>.npy)

A step = one pass of the hot path (blob bytes -> 128 cells + 128 proofs per blob) over one batch of
synthetic blobs that is already resident in HBM, through the device-pointer C ABI
(eth_kzg_amd_compute_cells_and_kzg_proofs_device).  One process per GPU; the batch is sharded by
contiguous blob index with no data-path collective; with N > 1 each step ends with one RCCL
all-gather of the proof vectors (48 B x 128 per blob) on the library's own communicator
(eth_kzg_amd_all_gather), which is the only exchange north_star names.
Weak scaling: the per-GPU batch is fixed (default 2048 blobs, batch-saturated as BASELINE.md section 3 asks); at N > 1
a --full run's JSON also carries `configs_strong`: BASELINE configs 4 and 5 AS WRITTEN (512 / 256 blobs in total, split N ways,
gathered), timed outside the headline region next to the same total on one GPU -- the strong-scaling numbers.

Rank 0 prints ONE JSON line.  A plain run does only what the headline needs: it builds the context (the widest tables),
warms up, times --steps steps, writes the outputs of the last step if --dump-outputs DIR is given, and prints `metric`,
`value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step` and the configuration.  Everything else runs with --full:
the correctness gate, the context-creation figures, `roofline`, per-stage times, the single-blob latency, `cpu_baseline`,
and at N = 1 a `configs` block (BASELINE.json's other configurations and the reference's own bench set,
crates/eip7594/benches/benchmark-mt.rs:36-113), at N > 1 the strong-scaling and device-list legs -- all measured in the
same process, outside the headline region.  The --no-* options switch single legs of a --full run off.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BYTES_PER_BLOB, CELLS, BYTES_PER_CELL = 131072, 128, 2048
ALG_BYTES_PER_BLOB = BYTES_PER_BLOB + CELLS * BYTES_PER_CELL + CELLS * 48  # 399,360 B
HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: 8.0 TB/s spec
VALU_INT_PEAK_GOPS = 34000.0     # measured on MI355X with tools/ubench.hip: integer VALU ops (v_mad_u64_u32,
                                 # v_addc_co_u32, ...) all issue at ~31-35 T lane-ops/s chip-wide
VALU_MIX_PEAK_TLOPS = 34.4      # measured issue ceiling of the point kernels' 12 : 4 multiply-add mix at 2 waves/SIMD (profiles/r3_ubench_issue.log), T lane-ops/s at 2.4 GHz
FP_MUL_PEAK_G = 82.2             # measured SUSTAINED rate of the signed 13x30-bit Montgomery multiplication with centred result (338 + 13
                                 # v_mad_i64_i32 as verbatim chains, fp30_mac.hpp) at the 2 waves/SIMD the point kernels hold:
                                 # tools/ubench_fp30 --sustained, profiles/archive/r5_ubench_fp30_sustained.log (14x29-bit form: 76.2 G/s)


def fp_mul_eq_per_blob(window_bits, linmap, batch_lanes=2048):
    """Fp multiplication equivalents this build spends per blob, counted in multiply-add passes of the signed 13-digit field's
    351 MACs (M = 1, squaring S = 273/351, fused pair a*b + c*d with one reduction F = 520/351; the cheap levels of the linear
    map still run in the 14-digit field and are counted with the same weights):
    stage D: 128 MSMs x 64 bases x W windows XYZZ mixed additions (6M + 2S + F);
    stages E+F as one compiled linear map (g1_linmap.hpp): `mulc` constant multiplications, each = the co-Z table of 8 odd
    multiples (a doubling with update 2M + 4S + F, 7 co-Z additions 4M + 2S, 8 lifts to the common Z with the beta multiple
    5M + S, 1M for the common Z) + 128 doublings (2M + 3S + F) + ~43 mixed additions (6M + 3S + F) + 1M; + its general
    additions (10M + 4S + F) and doublings.  From 1024 lanes on, every subtraction of the FK20 program shares the work of the
    addition of the same two values (g1_linmap.hpp: 548 pairs of its 3162 additions and subtractions): the second result of a
    pair costs S + F."""
    w = 2 * -(-128 // window_bits)  # gathered additions per (scalar, base): both 128-bit halves over ceil(128 / w) windows
    S, F = 273 / 351, 520 / 351
    madd, dbl, add, madd_jac = 6 + 2 * S + F, 2 + 3 * S + F, 10 + 4 * S + F, 6 + 3 * S + F
    mulc, adds, dbls = linmap
    table = (dbl + S) + 7 * (4 + 2 * S) + 8 * (5 + S) + 1
    pairs = 548 if (adds == 3162 and batch_lanes >= 1024) else 0
    return (128 * 64 * w * madd + mulc * (table + 128 * dbl + 43 * madd_jac + 1) + (adds - pairs) * add + pairs * (S + F) + dbls * dbl)


def synth_blobs(n, seed):
    """n valid blobs: every 32-byte element uniform in [0, 2^254) < r, deterministic in (seed)."""
    import numpy as np
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, 4096, 32), dtype=np.uint8)
    a[:, :, 0] &= 0x3F
    return a.reshape(n, BYTES_PER_BLOB)


def _host_cores():
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:  # a cgroup CPU quota caps the usable cores below the visible count (the GPU boxes: 256 visible, quota 16)
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            cores = max(1, min(cores, int(int(q) / int(per))))
    except Exception:
        pass
    return cores


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def _criterion(fn, warmup_s, samples, max_s):
    """criterion-like: warm up for warmup_s, then `samples` timed iterations (cut short at max_s); returns the sample times."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warmup_s:
        fn()
    ts, t0 = [], time.perf_counter()
    while len(ts) < samples and (time.perf_counter() - t0 < max_s or len(ts) < 3):
        t1 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t1)
    return ts


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def _oracle_uses_adx():
    try:
        import ctypes
        import oracle_lib
        return bool(ctypes.CDLL(oracle_lib._SO).oracle_fp_mul_uses_adx())
    except Exception:
        return False


def cpu_baseline(blobs, gpu_first=None, extra=None):
    """Time the CPU oracle (C restatement of the reference algorithm: FK20, width-8 window tables, batched affine
    additions; portable unsigned __int128 field arithmetic, NOT blst's assembly) on this box's host cores with the
    criterion-like protocol of BASELINE.md section 3 (3 s warm-up, 30 samples, median and min), in two arrangements:
      * blob-parallel: one single-threaded prover per host core, distinct blobs (the strongest CPU arrangement for a
        throughput metric); a sample = one round of `cores` blobs                       -> cpu_baseline.value
      * rayon-like: one blob at a time with OpenMP threads over the axes maybe_rayon parallelises
        (fk20/batch_toeplitz.rs:50,68,95,104,114; polynomial/src/fft.rs:72,119)        -> cpu_baseline.rayon_like
    plus the single-threaded rate (8 samples: a blob takes ~0.3 s) and, if `extra` is given, one CPU sample each of
    BASELINE configs 3 and 5."""
    import concurrent.futures as cf
    cores = _host_cores()
    import oracle_lib
    fp_mul_ab = {}
    try:
        # native builds of the same sources for this host (the prebuilt liboracle.so is generic x86-64), in BOTH forms of the Fp
        # multiplication: gcc's code for the portable unsigned __int128 product scanning (with -march=native it already uses mulx)
        # and -DORACLE_ADX (oracle/field.c: mont_mul6_adx, mulx + two explicit carry chains; checked against the portable form on
        # 10^6 pairs by tests/test_oracle_units.py).  Which is faster depends on the CPU (measured: the explicit form +6 % on the
        # build container's CPU, -9 % on the GPU boxes' EPYC 9575F), so both are timed on two blobs and the FASTER one is the baseline.
        src = [os.path.join(ROOT, "oracle", f) for f in ("field.c", "g1.c", "pairing.c", "sha256.c", "kzg.c")]
        best = None
        # a private directory per process (a predictable shared path in /tmp is a pre-creation hazard on a multi-user box,
        # and concurrent ranks raced writing the file another one was loading)
        import tempfile
        native_dir = tempfile.mkdtemp(prefix="kzg_oracle_native_")
        built = {}
        for tag, flags in (("portable", []), ("adx", ["-DORACLE_ADX"])):
            so = built[tag] = os.path.join(native_dir, "liboracle_native_%s.so" % tag)
            subprocess.check_call(["gcc", "-O3", "-march=native", *flags, "-fopenmp", "-fPIC", "-std=gnu11", "-shared", "-o", so] + src, stderr=subprocess.DEVNULL)
            oracle_lib._SO = so
            o1 = oracle_lib.Oracle(use_precomp=True, threads=1)
            o1.compute_cells_and_kzg_proofs(blobs[0])
            t0 = time.perf_counter()
            o1.compute_cells_and_kzg_proofs(blobs[1 % len(blobs)])
            o1.compute_cells_and_kzg_proofs(blobs[2 % len(blobs)])
            fp_mul_ab[tag] = round((time.perf_counter() - t0) / 2 * 1e3, 1)
            o1.close()
            if best is None or fp_mul_ab[tag] < fp_mul_ab[best]:
                best = tag
        oracle_lib._SO = built[best]
        fp_mul_ab["used"] = best
    except Exception as e:  # noqa: BLE001 -- never silent: the record says which build was timed
        oracle_lib._SO = os.path.join(ROOT, "oracle", "liboracle.so")
        fp_mul_ab = {"used": "prebuilt generic x86-64 liboracle.so (the native build failed: %s)" % (repr(e)[:200],)}
    from oracle_lib import Oracle
    # --- rayon-like (intra-blob parallel) at all usable cores
    o = Oracle(use_precomp=True, threads=cores)
    k = [0]

    def one_rayon():
        o.compute_cells_and_kzg_proofs(blobs[k[0] % len(blobs)])
        k[0] += 1
    ts = _criterion(one_rayon, 3.0, 30, 6.0)
    rayon = {"value": 1.0 / _median(ts), "best": 1.0 / min(ts), "threads": cores, "samples": len(ts),
             "note": "one blob at a time, OpenMP over the maybe_rayon axes; median of the samples"}
    o.close()
    # --- blob-parallel over all cores (ctypes releases the GIL; the context is read-only while computing)
    o = Oracle(use_precomp=True, threads=1)
    ref_cells, ref_proofs = o.compute_cells_and_kzg_proofs(blobs[0])
    agrees = None
    if gpu_first is not None:  # the oracle doubles as the checker here: the GPU's bytes for blob 0 of the timed batch
        agrees = (b"".join(ref_cells) == gpu_first[0]) and (b"".join(ref_proofs) == gpu_first[1])
        if not agrees:
            raise SystemExit("bench.py: GPU cells/proofs of blob 0 differ from the CPU oracle")
    ts1 = _criterion(lambda: o.compute_cells_and_kzg_proofs(blobs[1 % len(blobs)]), 1.0, 8, 4.0)
    single_thread = 1.0 / _median(ts1)
    ex = cf.ThreadPoolExecutor(max_workers=cores)

    def one_round():
        list(ex.map(lambda w: o.compute_cells_and_kzg_proofs(blobs[w % len(blobs)]), range(cores)))
    tsp = _criterion(one_round, 3.0, 30, 12.0)
    par, par_best = cores / _median(tsp), cores / min(tsp)
    out_extra = {}
    if extra is not None:  # one CPU sample each of configs 3 and 5 (seconds each: stated deviation from the 30-sample protocol)
        try:
            C_, I_, L_, P_ = extra["verify"]
            ov = Oracle(use_precomp=True, threads=cores)
            t0 = time.perf_counter()
            ok = ov.verify_cell_kzg_proof_batch(C_, I_, L_, P_)
            out_extra["config3_verify_8192_cells_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            out_extra["config3_verified"] = bool(ok)
            ov.close()
            idx, cells = extra["recover"]
            t0 = time.perf_counter()
            list(ex.map(lambda w: o.recover_cells_and_kzg_proofs(idx, cells), range(cores)))
            out_extra["config5_recover_blobs_per_s"] = round(cores / (time.perf_counter() - t0), 2)
            out_extra["note"] = "one sample each (a verification of 8192 cells and a round of recoveries take seconds on the CPU)"
        except Exception as e:  # the baseline of the side configs must never sink the headline record
            out_extra["error"] = repr(e)
    # the reference's own criterion shapes (benchmark-mt.rs:36-113, benchmark-st.rs:36-48), each by the criterion-like protocol
    # (shorter: 1 s warm-up, <= 12 samples): BASELINE.json config 1 is `blob_to_kzg_commitment` on one blob, single thread
    shapes = {}
    try:
        b0 = blobs[0]
        ts = _criterion(lambda: o.blob_to_kzg_commitment(b0), 1.0, 12, 4.0)
        shapes["config1_blob_to_kzg_commitment_one_blob_single_thread_ms"] = {"median": round(_median(ts) * 1e3, 2), "min": round(min(ts) * 1e3, 2), "samples": len(ts)}
        om = Oracle(use_precomp=True, threads=cores)
        ts = _criterion(lambda: om.blob_to_kzg_commitment(b0), 1.0, 12, 3.0)
        shapes["blob_to_kzg_commitment_one_blob_all_cores_ms"] = {"median": round(_median(ts) * 1e3, 2), "min": round(min(ts) * 1e3, 2), "samples": len(ts), "threads": cores}
        if extra is not None and "verify128" in extra:
            C1, I1, L1, P1 = extra["verify128"]
            assert om.verify_cell_kzg_proof_batch(C1, I1, L1, P1) is True
            for nm, orc, thr in (("verify_128_cells_one_commitment_single_thread_ms", o, 1), ("verify_128_cells_one_commitment_all_cores_ms", om, cores)):
                ts = _criterion(lambda: orc.verify_cell_kzg_proof_batch(C1, I1, L1, P1), 1.0, 12, 4.0)
                shapes[nm] = {"median": round(_median(ts) * 1e3, 2), "min": round(min(ts) * 1e3, 2), "samples": len(ts), "threads": thr}
            # many such verifications at once: one single-threaded verifier per core (how the reference gets verification throughput)
            t0 = time.perf_counter()
            rounds = 3
            for _ in range(rounds):
                list(ex.map(lambda w: o.verify_cell_kzg_proof_batch(C1, I1, L1, P1), range(cores)))
            shapes["verify_128_cells_verifications_per_s_all_cores"] = round(rounds * cores / (time.perf_counter() - t0), 1)
        if extra is not None and "recover" in extra:
            idx, cells_h = extra["recover"]
            for nm, orc, thr in (("recover_one_blob_half_missing_single_thread_ms", o, 1), ("recover_one_blob_half_missing_all_cores_ms", om, cores)):
                ts = _criterion(lambda: orc.recover_cells_and_kzg_proofs(idx, cells_h), 1.0, 8, 4.0)
                shapes[nm] = {"median": round(_median(ts) * 1e3, 2), "min": round(min(ts) * 1e3, 2), "samples": len(ts), "threads": thr}
        om.close()
        ts = []
        for _ in range(3):  # "Initialize context" (benchmark-mt.rs:103-113): width-8 tables for the 128 x 64 FK20 bases, on all cores
            t0 = time.perf_counter()
            oc = Oracle(use_precomp=True, threads=cores)
            ts.append(time.perf_counter() - t0)
            oc.close()
        shapes["initialize_context_s"] = {"median": round(_median(ts), 3), "min": round(min(ts), 3), "samples": 3, "threads": cores}
        shapes["note"] = "C oracle (portable __int128 arithmetic, not blst assembly); medians of criterion-like samples, context built once outside unless timed"
    except Exception as e:  # the side shapes must never sink the headline record
        shapes["error"] = repr(e)
    ex.shutdown()
    o.close()
    best_value, best_cores = (par, cores) if par >= rayon["value"] else (rayon["value"], cores)
    return {"value": best_value, "unit": "blobs/s", "cores": best_cores, "kind": "port", "cpu_model": _cpu_model(),
            "protocol": "criterion-like (BASELINE.md section 3): 3 s warm-up, 30 timed samples, median; context built once outside",
            "fp_mul": ("ADX/BMI2 (mulx, two carry chains; oracle/field.c: mont_mul6_adx)" if _oracle_uses_adx() else "gcc's -march=native code for the portable unsigned __int128 form (it uses mulx)"),
            "fp_mul_forms_ms_per_blob_single_thread": fp_mul_ab,
            "sample": f"C oracle (width-8 tables; native build; Fp multiplication: the faster on this CPU of the explicit ADX/BMI2 form and gcc's own "
                      f"code for the __int128 form -- {fp_mul_ab}; not blst's hand-scheduled assembly) on {cores} usable host "
                      f"cores: (a) blob-parallel, one single-threaded prover per core, {len(tsp)} rounds of {cores} distinct "
                      f"synthetic blobs, median {_median(tsp):.3f} s per round = {par:.1f} blobs/s (best {par_best:.1f}); (b) one blob "
                      f"at a time with OpenMP over the maybe_rayon axes, {rayon['samples']} samples = {rayon['value']:.1f} blobs/s; "
                      f"single thread ({len(ts1)} samples) = {single_thread:.2f} blobs/s",
            "gpu_matches_oracle_on_blob0": agrees,
            "blob_parallel": {"value": par, "best": par_best, "threads": cores, "samples": len(tsp)},
            "single_thread": single_thread,
            "rayon_like": rayon,
            "other_configs_cpu": out_extra,
            "reference_bench_shapes_cpu": shapes}


def _mark(what):
    if os.environ.get("KZG_BENCH_VERBOSE"):
        print(f"[bench {time.strftime('%H:%M:%S')}] {what}", file=sys.stderr, flush=True)


def side_configs(ctx, kzg, torch, dev, blobs_h, ctx_times):
    """BASELINE.json's other configurations and the reference's own bench set (benchmark-mt.rs:36-113), on this GPU, after
    the headline region: medians of a few runs each, inputs resident where the entry point is device-resident."""
    import numpy as np
    out = {}
    stream = torch.cuda.Stream(device=dev)

    def dev_rate(nb, fn_name="compute"):
        d_b = torch.from_numpy(blobs_h[:nb]).to(dev)
        d_c = torch.empty(nb * CELLS * BYTES_PER_CELL, dtype=torch.uint8, device=dev)
        d_p = torch.empty(nb * CELLS * 48, dtype=torch.uint8, device=dev)
        ts = []
        for it in range(7):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                if fn_name == "compute":
                    ctx.compute_cells_and_kzg_proofs_device(nb, d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), want_status=False, stream=stream.cuda_stream)
                elif fn_name == "cells":
                    ctx.compute_cells_and_kzg_proofs_device(nb, d_b.data_ptr(), d_c.data_ptr(), 0, want_status=False, stream=stream.cuda_stream)
                else:
                    ctx.blob_to_kzg_commitment_device(nb, d_b.data_ptr(), d_p.data_ptr(), want_status=False, stream=stream.cuda_stream)
            torch.cuda.synchronize(dev)
            if it >= 2:
                ts.append(time.perf_counter() - t0)
        return nb / _median(ts), _median(ts) * 1e3, (d_b, d_c, d_p)

    B = blobs_h.shape[0]
    _mark("side configs: device rates")
    r64, ms64, _ = dev_rate(min(64, B))
    out["config4_per_gpu_share_64_blobs"] = {"blobs_per_s": round(r64), "ms": round(ms64, 2), "form": "device-resident"}
    r256, ms256, _ = dev_rate(min(256, B))
    out["batch_256_blobs_on_one_gpu"] = {"blobs_per_s": round(r256), "ms": round(ms256, 2), "form": "device-resident"}
    r512, ms512, _ = dev_rate(min(512, B))
    out["config4_512_blobs_on_one_gpu"] = {"blobs_per_s": round(r512), "ms": round(ms512, 2), "form": "device-resident"}
    rc, msc, _ = dev_rate(B, "cells")
    out["compute_cells_only"] = {"blobs_per_s": round(rc), "ms": round(msc, 2), "blobs": B, "form": "device-resident"}
    rk, msk, _ = dev_rate(B, "commit")
    out["blob_to_kzg_commitment"] = {"commitments_per_s": round(rk), "ms": round(msk, 2), "blobs": B, "form": "device-resident"}
    # the reference's ABI: host pointers (pageable memory in, 256 caller buffers per blob out)
    _mark("side configs: host-pointer ABI")
    bufs = ctx.host_batch_buffers(B)
    ctx.compute_cells_and_kzg_proofs_batch_np(blobs_h, bufs)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        ctx.compute_cells_and_kzg_proofs_batch_np(blobs_h, bufs)
        ts.append(time.perf_counter() - t0)
    out["abi_host_pointer_batch"] = {"blobs_per_s": round(B / _median(ts)), "ms": round(_median(ts) * 1e3, 2), "blobs": B,
                                     "entry": "eth_kzg_amd_compute_cells_and_kzg_proofs_batch (PCIe both ways, gather and scatter included)"}
    # the same entry point from TWO caller threads, each with its own batch and buffers: one call's gather and upload run under the
    # other call's MSMs (the context has three independent work sets) -- what a host that pipelines its calls gets
    import threading as _th
    bufs2 = ctx.host_batch_buffers(B)
    ctx.compute_cells_and_kzg_proofs_batch_np(blobs_h, bufs2)

    def _caller(bf, k):
        for _ in range(k):
            ctx.compute_cells_and_kzg_proofs_batch_np(blobs_h, bf)
    tt = [_th.Thread(target=_caller, args=(bf, 3)) for bf in (bufs, bufs2)]
    t0 = time.perf_counter()
    for t in tt:
        t.start()
    for t in tt:
        t.join()
    dt2 = time.perf_counter() - t0
    out["abi_host_pointer_batch_two_callers"] = {"blobs_per_s": round(6 * B / dt2), "ms_per_call": round(dt2 / 6 * 1e3, 2), "blobs": B,
                                                 "entry": "eth_kzg_amd_compute_cells_and_kzg_proofs_batch from two threads, three calls each"}
    del bufs2
    one = blobs_h[0].tobytes()
    ctx.compute_cells_and_kzg_proofs(one)
    ts = []
    for _ in range(9):
        t0 = time.perf_counter()
        ctx.compute_cells_and_kzg_proofs(one)
        ts.append(time.perf_counter() - t0)
    out["abi_single_call_latency_ms"] = {"ms": round(_median(ts) * 1e3, 3), "entry": "eth_kzg_compute_cells_and_kzg_proofs (ctypes wrapper included)"}
    # config 3: verify 64 blobs x 128 cells (host-pointer ABI; its transcript hash needs the bytes on the host anyway)
    _mark("side configs: config 3")
    nb = 64
    d_b = torch.from_numpy(blobs_h[:nb]).to(dev)
    d_c = torch.empty(nb * CELLS * BYTES_PER_CELL, dtype=torch.uint8, device=dev)
    d_p = torch.empty(nb * CELLS * 48, dtype=torch.uint8, device=dev)
    ctx.compute_cells_and_kzg_proofs_device(nb, d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr())
    cells = d_c.cpu().numpy().tobytes()
    proofs = d_p.cpu().numpy().tobytes()
    _, comms = ctx.blob_to_kzg_commitment_batch([blobs_h[b].tobytes() for b in range(nb)])
    C_, I_, L_, P_ = [], [], [], []
    for b in range(nb):
        for k in range(CELLS):
            j = b * CELLS + k
            C_.append(comms[b]); I_.append(k); L_.append(cells[BYTES_PER_CELL * j:BYTES_PER_CELL * (j + 1)]); P_.append(proofs[48 * j:48 * (j + 1)])
    run_verify = ctx.prepare_verify_cell_kzg_proof_batch(C_, I_, L_, P_)  # pointer tables built once, as a C caller holds them
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        ok = run_verify()
        ts.append(time.perf_counter() - t0)
        assert ok
    P2 = list(P_)
    P2[77] = P_[78]
    assert ctx.verify_cell_kzg_proof_batch(C_, I_, L_, P2) is False
    out["config3_verify_64x128_cells"] = {"ms": round(_median(ts) * 1e3, 2), "cells": len(L_), "cells_per_s": round(len(L_) / _median(ts)),
                                          "entry": "eth_kzg_verify_cell_kzg_proof_batch (host pointers, 17.6 MB of input; tampered proof -> false checked)"}
    # the same batch with cells and proofs where the prover left them, in HBM (eth_kzg_amd_verify_cell_kzg_proof_batch_device): the GPU's part
    # reads them in place, only the transcript's bytes come down (in chunks, under the hash)
    try:
        d_comm = torch.frombuffer(bytearray(b"".join(comms)), dtype=torch.uint8).to(dev).view(nb, 1, 48).expand(nb, CELLS, 48).contiguous().view(-1)
        d_idx = torch.arange(CELLS, dtype=torch.int64, device=dev).repeat(nb)
        torch.cuda.synchronize(dev)
        tsd = []
        for it in range(7):
            t0 = time.perf_counter()
            okd = ctx.verify_cell_kzg_proof_batch_device(nb * CELLS, d_comm.data_ptr(), d_idx.data_ptr(), d_c.data_ptr(), d_p.data_ptr())
            if it >= 1:
                tsd.append(time.perf_counter() - t0)
            assert okd is True
        out["config3_verify_64x128_cells_device_resident"] = {"ms": round(_median(tsd) * 1e3, 2), "cells": nb * CELLS,
                                                              "entry": "eth_kzg_amd_verify_cell_kzg_proof_batch_device (cells and proofs stay in HBM for the GPU's part; "
                                                                       "17.6 MB come down in chunks for the SHA-256 transcript, 7.2 ms of one host core = the floor)"}
    except Exception as e:  # a side figure must not cost the record
        out["config3_verify_64x128_cells_device_resident"] = {"error": repr(e)}
    # config 5: recover 256 blobs at 50 % erasure, device-resident form; and its per-GPU share on 8 GPUs (32 blobs)
    _mark("side configs: config 5")
    for nb, key in ((min(256, B), "config5_recover_256_blobs_half_erased"), (32, "config5_per_gpu_share_32_blobs")):
        d_b = torch.from_numpy(blobs_h[:nb]).to(dev)
        d_c = torch.empty(nb * CELLS * BYTES_PER_CELL, dtype=torch.uint8, device=dev)
        d_p = torch.empty(nb * CELLS * 48, dtype=torch.uint8, device=dev)
        ctx.compute_cells_and_kzg_proofs_device(nb, d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr())
        erased = d_c.view(nb, CELLS, BYTES_PER_CELL).clone()
        erased[:, 1::2, :] = 0xFF
        d_oc, d_op = torch.empty_like(d_c), torch.empty_like(d_p)
        idx = list(range(0, CELLS, 2))
        ts = []
        for it in range(5):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            st = ctx.recover_cells_and_kzg_proofs_device(nb, erased.data_ptr(), [idx] * nb, d_oc.data_ptr(), d_op.data_ptr())
            torch.cuda.synchronize(dev)
            if it >= 1:
                ts.append(time.perf_counter() - t0)
        assert st == [0] * nb and torch.equal(d_oc, d_c) and torch.equal(d_op, d_p), "recovery does not reproduce the prover's output"
        out[key] = {"ms": round(_median(ts) * 1e3, 2), "blobs_per_s": round(nb / _median(ts)), "blobs": nb, "form": "device-resident"}
    recover_one = (list(range(0, CELLS, 2)), [cells[BYTES_PER_CELL * k:BYTES_PER_CELL * (k + 1)] for k in range(0, CELLS, 2)])
    # the reference's own criterion shapes (benchmark-mt.rs:51-101): one blob's 128 cells against one commitment, and the
    # worst-case recovery of one blob from its first 64 cells -- both through the reference's C entry points, latency per call
    run_v1 = ctx.prepare_verify_cell_kzg_proof_batch(C_[:CELLS], I_[:CELLS], L_[:CELLS], P_[:CELLS])
    ts = []
    for it in range(12):
        t0 = time.perf_counter()
        ok = run_v1()
        if it >= 2:
            ts.append(time.perf_counter() - t0)
        assert ok
    out["reference_bench_verify_128_cells_one_commitment"] = {"ms": round(_median(ts) * 1e3, 3), "entry": "eth_kzg_verify_cell_kzg_proof_batch"}
    # many independent verifications of that shape in ONE call (eth_kzg_amd_verify_cell_kzg_proof_batch_many): 64 distinct
    # problems (one per blob) repeated to 1024, one of them tampered; and the same problems from 4 host threads through the
    # single-call entry point (engine lanes)
    _mark("side configs: verify_many")
    probs = [(C_[b * CELLS:(b + 1) * CELLS], I_[b * CELLS:(b + 1) * CELLS], L_[b * CELLS:(b + 1) * CELLS], P_[b * CELLS:(b + 1) * CELLS]) for b in range(nb)]
    many = [probs[j % nb] for j in range(1024)]
    run_many = ctx.prepare_verify_cell_kzg_proof_batch_many(many)
    ver, stt = run_many()
    assert stt == [0] * 1024 and ver == [True] * 1024, "verify_many verdicts"
    ts = []
    for it in range(5):
        t0 = time.perf_counter()
        run_many()
        if it >= 1:
            ts.append(time.perf_counter() - t0)
    # the same call with ONE tampered proof among the 1024 problems: the folded pairing check of the pass fails and every
    # problem is checked on its own (the cost of a call that contains an invalid proof)
    bad = list(many[77][3]); bad[5] = many[78][3][5]
    many_bad = list(many)
    many_bad[77] = (many[77][0], many[77][1], many[77][2], bad)
    run_bad = ctx.prepare_verify_cell_kzg_proof_batch_many(many_bad)
    ver, stt = run_bad()
    assert stt == [0] * 1024 and ver == [j != 77 for j in range(1024)], "verify_many verdicts (one tampered problem)"
    tb = []
    for it in range(3):
        t0 = time.perf_counter()
        run_bad()
        tb.append(time.perf_counter() - t0)
    # ... and with EIGHT tampered problems spread over the call
    bad_at = [3, 77, 200, 201, 512, 700, 901, 1023]
    many_bad8 = list(many)
    for j in bad_at:
        pj = list(many[j][3]); pj[9] = many[(j + 1) % nb][3][9]
        many_bad8[j] = (many[j][0], many[j][1], many[j][2], pj)
    run_bad8 = ctx.prepare_verify_cell_kzg_proof_batch_many(many_bad8)
    ver, stt = run_bad8()
    assert stt == [0] * 1024 and ver == [j not in bad_at for j in range(1024)], "verify_many verdicts (eight tampered problems)"
    tb8 = []
    for it in range(3):
        t0 = time.perf_counter()
        run_bad8()
        tb8.append(time.perf_counter() - t0)
    out["verify_many_1024_x_128_cells"] = {"ms": round(_median(ts) * 1e3, 2), "verifications_per_s": round(1024 / _median(ts)), "cells_per_s": round(1024 * CELLS / _median(ts)),
                                           "with_one_invalid_proof_ms": round(_median(tb) * 1e3, 2), "with_one_invalid_proof_verifications_per_s": round(1024 / _median(tb)),
                                           "with_eight_invalid_proofs_ms": round(_median(tb8) * 1e3, 2), "with_eight_invalid_proofs_verifications_per_s": round(1024 / _median(tb8)),
                                           "entry": "eth_kzg_amd_verify_cell_kzg_proof_batch_many (host pointers: 275 MB of input per call, staging and 1024 transcript hashes on the "
                                                    "host threads included; a call this large runs as three concurrent parts on the pass slots; all problems valid: ONE folded pairing check per part; with invalid proofs in the call: "
                                                    "the wrong problems are searched by folding sub-ranges of the resident weighted sums, one pairing per probe "
                                                    "on the host threads; verdicts checked)"}
    _mark("side configs: single verifications from many threads")
    import threading
    for n_thr, key in ((4, "verify_128_cells_from_4_threads"), (32, "verify_128_cells_from_32_threads")):
        runs_t = [ctx.prepare_verify_cell_kzg_proof_batch(*probs[b % nb]) for b in range(n_thr)]
        reps = 60

        def hammer(r):
            for _ in range(reps):
                assert r()
        for r in runs_t[:2]:
            r()
        # an untimed round first: the pass slots get their arenas, the host pool its threads, on first use
        warm = [threading.Thread(target=lambda r=r: [r() for _ in range(4)]) for r in runs_t]
        for t in warm:
            t.start()
        for t in warm:
            t.join()
        ths = [threading.Thread(target=hammer, args=(r,)) for r in runs_t]
        # the interpreter's cyclic garbage collector is held off for the timed round: by now this process holds millions of Python
        # objects (the 1024-problem calls' lists), one full collection takes ~35 ms WITH the GIL -- every caller thread needs the
        # GIL to return from its call, so all four stood still for it once per round (a fifth of the 4-thread round's 220 ms;
        # traced: four calls of 39 ms at the same instant, the other 236 at 3.7 ms).  A harness artefact, not library time.
        import gc
        gc.collect()
        gc.disable()
        try:  # (a failed assert in a hammer thread must not leave the collector off for the rest of the record: ADVICE r4)
            t0 = time.perf_counter()
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            dtt = time.perf_counter() - t0
        finally:
            gc.enable()
        # the same round with the collector ON: what a Python host that does not hold it off sees; the library's share of any
        # round-to-round change is the figure above, the difference between the two is the harness
        ths = [threading.Thread(target=hammer, args=(r,)) for r in runs_t]
        t0 = time.perf_counter()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        dtt_gc = time.perf_counter() - t0
        out[key] = {"verifications_per_s": round(n_thr * reps / dtt),
                    "verifications_per_s_with_python_gc_enabled": round(n_thr * reps / dtt_gc),
                    "entry": f"eth_kzg_verify_cell_kzg_proof_batch from {n_thr} host threads on one context: one caller at a time takes the latency "
                             "path, callers that arrive meanwhile are combined into many-verification passes (three pass slots, short-chain form); "
                             "the harness's own garbage collector held off during the timed round (one full collection of this process's "
                             "object graph = 35 ms under the GIL); the second figure is the same round with the collector on"}
    _mark("side configs: recover one")
    half_idx, half_cells = list(range(CELLS // 2)), L_[:CELLS // 2]
    ts = []
    for it in range(9):
        t0 = time.perf_counter()
        rc, rp = ctx.recover_cells_and_kzg_proofs(half_idx, half_cells)
        if it >= 2:
            ts.append(time.perf_counter() - t0)
    assert rc == L_[:CELLS] and rp == P_[:CELLS], "single-blob recovery does not reproduce the prover's output"
    out["reference_bench_recover_one_blob_half_missing"] = {"ms": round(_median(ts) * 1e3, 3), "entry": "eth_kzg_recover_cells_and_kzg_proofs (ctypes wrapper included)"}
    # context creation (the reference's "Initialize context" bench): cold = first context of the process (measured by the
    # caller), warm = another context while one is alive (tables shared), fresh = after every context was closed
    _mark("side configs: warm context, fresh process")
    t0 = time.perf_counter()
    c2 = kzg.DASContext(use_precomp=True, device=ctx.device_index)
    warm = time.perf_counter() - t0
    c2.close()
    # a fresh process that loads nothing but the library (no torch): process start -> context -> first result, by its own clock
    cold = None
    try:
        script = ("import time,os,sys,importlib,json\n"
                  "t_imp=time.time()\n"
                  "import psutil\n"
                  "t0=psutil.Process().create_time()\n"
                  f"sys.path.insert(0,{ROOT!r})\n"
                  "k=importlib.import_module('rust-eth-kzg_amd')\n"
                  "k.load_library(); t_lib=time.time()\n"
                  f"c=k.DASContext(True,device={ctx.device_index},wait_tables=False); t_new=time.time()\n"
                  "blob=bytes(131072)\n"
                  "c.compute_cells_and_kzg_proofs(blob); t_first=time.time()\n"
                  "print(json.dumps({'python_start_s':round(t_imp-t0,3),'library_loaded_s':round(t_lib-t0,3),'constructor_returned_s':round(t_new-t0,3),"
                  "'first_result_s':round(t_first-t0,3),'start_table_window_bits':c.window_bits()}))\n"
                  "sys.stdout.flush(); os._exit(0)\n")  # (no wait for this child's own wide tables)
        r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=120)
        cold = json.loads(r.stdout.strip().splitlines()[-1])
        cold["note"] = "seconds since the creation of a fresh process (no torch): interpreter, dlopen, HIP runtime start (~0.45 s), start tables, one compute_cells_and_kzg_proofs"
    except Exception as e:
        cold = {"error": repr(e)}
    try:  # the same from a plain C consumer of the shared library (tools/first_result): no interpreter in front
        tool = os.path.join(ROOT, "tools", "first_result")
        subprocess.run(["make", "-C", tool], capture_output=True, timeout=120)
        r = subprocess.run([os.path.join(tool, "run")], capture_output=True, text=True, timeout=120)
        cold_c = json.loads(r.stdout.strip().splitlines()[-1])
        cold_c["note"] = "seconds since main() of a C program linked against libc_eth_kzg.so: HIP runtime start, start tables, one eth_kzg_compute_cells_and_kzg_proofs"
    except Exception as e:
        cold_c = {"error": repr(e)}
    out["context_creation_s"] = dict(ctx_times, warm_tables_shared=round(warm, 3), fresh_process=cold, fresh_c_process=cold_c,
                                     note="first context of the process: eth_kzg_das_context_new returns on the start tables (GLV width 8 + plain "
                                          "width 8, 3.7 GB; HIP runtime start ~0.45 s included), first_result = one compute_cells_and_kzg_proofs "
                                          "on them, wide tables (hipMalloc of ~250 GB: seconds of driver time, + ~0.9 s of build) swapped in by a helper thread")
    return out, {"verify": (C_, I_, L_, P_), "recover": recover_one, "verify128": (C_[:CELLS], I_[:CELLS], L_[:CELLS], P_[:CELLS])}


class _Harness:
    """The harness's own collectives (timing maxima, agreement flags, checksums, the torch-side all-gather): on the GPU with the
    "nccl" backend; through CPU copies with "gloo" -- the REHEARSAL mode (KZG_BENCH_REHEARSAL=1: N ranks share GPU 0, each with
    a small table budget), which exists so that the N > 1 code paths (launcher, seeds, slices, gather checks, strong legs) can
    run on a one-GPU box.  RCCL refuses two ranks on one GPU, so the rehearsal never measures an exchange."""
    def __init__(self, torch, dist, dev, rehearsal):
        self.torch, self.dist, self.dev, self.rehearsal = torch, dist, dev, rehearsal

    def _c(self, t):
        return t.cpu() if self.rehearsal else t

    def all_reduce(self, t, op):
        c = self._c(t)
        self.dist.all_reduce(c, op=op)
        if self.rehearsal:
            t.copy_(c)
        return t

    def all_gather_into(self, out, local):
        if not self.rehearsal:
            self.dist.all_gather_into_tensor(out, local.reshape(-1))
            return out
        self.torch.cuda.synchronize(self.dev)
        co = self.torch.empty(out.numel(), dtype=out.dtype)
        self.dist.all_gather_into_tensor(co, local.reshape(-1).cpu())
        out.copy_(co)
        return out

    def barrier(self):
        self.dist.barrier()


def strong_configs(ctx, sharding, torch, dist, dev, world, rank, lib_comm, stream, hz):
    """BASELINE.json configs 4 and 5 AS WRITTEN -- a fixed total (512 blobs to prove, 256 half-erased blobs to recover) cut
    into contiguous slices over the N ranks, each pass ending with the all-gather -- timed outside the headline region,
    beside the same total on ONE GPU (every rank runs that leg on its own GPU; rank 0's figure is reported).  These are the
    strong-scaling numbers; the headline is weak scaling.  Each pass is timed on its own (barrier, run, local sync, MAX over
    ranks): a 512-blob job is one pass, not a pipeline.  The gathered bytes are checked against the one-GPU run."""
    out = {}

    def fence():
        torch.cuda.synchronize(dev)
        if world > 1:
            hz.barrier()
        torch.cuda.synchronize(dev)

    def gather(local, full):
        if world == 1 and not lib_comm:
            full.copy_(local)
        elif lib_comm:
            ctx.all_gather(local.data_ptr(), full.data_ptr(), local.numel(), stream.cuda_stream)
        else:
            hz.all_gather_into(full, local)

    def timed(run, reps=7, skip=2):
        ts = []
        for it in range(reps):
            fence()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                run()
            torch.cuda.synchronize(dev)
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            if world > 1:
                hz.all_reduce(t, dist.ReduceOp.MAX)
            if it >= skip:
                ts.append(float(t.item()))
        return _median(ts)

    def agree(flag):
        t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=dev)
        if world > 1:
            hz.all_reduce(t, dist.ReduceOp.MIN)
        return bool(int(t.item()))

    PB, CB = CELLS * 48, CELLS * BYTES_PER_CELL
    for total, key, recover in ((512, "config4_compute_512_blobs", False), (256, "config5_recover_256_blobs_half_erased", True)):
        blobs_all = torch.from_numpy(synth_blobs(total, seed=0x4B5A47)).to(dev)  # the same batch on every rank
        lo, hi = sharding.shard_bounds(total, world, rank)
        per = -(-total // world)  # slabs are padded to the largest slice so that one fixed-size all-gather does the exchange
        nb = hi - lo
        ref_c = torch.empty(total * CB, dtype=torch.uint8, device=dev)
        ref_p = torch.empty(total * PB, dtype=torch.uint8, device=dev)
        ctx.compute_cells_and_kzg_proofs_device(total, blobs_all.data_ptr(), ref_c.data_ptr(), ref_p.data_ptr())
        loc_c = torch.zeros(per * CB, dtype=torch.uint8, device=dev)
        loc_p = torch.zeros(per * PB, dtype=torch.uint8, device=dev)
        all_c = torch.empty(world * per * CB, dtype=torch.uint8, device=dev)
        all_p = torch.empty(world * per * PB, dtype=torch.uint8, device=dev)
        if recover:
            erased = ref_c.view(total, CELLS, BYTES_PER_CELL).clone()
            erased[:, 1::2, :] = 0xFF  # never read: only the cells named in `present` are
            idx = list(range(0, CELLS, 2))
            one_c, one_p = torch.empty_like(ref_c), torch.empty_like(ref_p)

            def one_gpu():
                ctx.recover_cells_and_kzg_proofs_device(total, erased.data_ptr(), [idx] * total, one_c.data_ptr(), one_p.data_ptr(), stream=stream.cuda_stream)

            def sliced(full_output):
                if nb:
                    ctx.recover_cells_and_kzg_proofs_device(nb, erased[lo:hi].data_ptr(), [idx] * nb, loc_c.data_ptr(), loc_p.data_ptr(), stream=stream.cuda_stream)
                gather(loc_p, all_p)
                if full_output:
                    gather(loc_c, all_c)
        else:
            one_c, one_p = torch.empty_like(ref_c), torch.empty_like(ref_p)

            def one_gpu():
                ctx.compute_cells_and_kzg_proofs_device(total, blobs_all.data_ptr(), one_c.data_ptr(), one_p.data_ptr(), want_status=False, stream=stream.cuda_stream)

            def sliced(full_output):
                if nb:
                    ctx.compute_cells_and_kzg_proofs_device(nb, blobs_all[lo:hi].data_ptr(), loc_c.data_ptr(), loc_p.data_ptr(), want_status=False, stream=stream.cuda_stream)
                gather(loc_p, all_p)
                if full_output:
                    gather(loc_c, all_c)
        t_one = timed(one_gpu)
        t_p = timed(lambda: sliced(False))
        t_full = timed(lambda: sliced(True))
        torch.cuda.synchronize(dev)
        # the gathered slabs, un-padded, must be the one-GPU result byte for byte -- on every rank
        same = torch.equal(one_p, ref_p) and torch.equal(one_c, ref_c)
        for r in range(world):
            rlo, rhi = sharding.shard_bounds(total, world, r)
            same = same and torch.equal(all_p[r * per * PB: r * per * PB + (rhi - rlo) * PB], ref_p[rlo * PB: rhi * PB])
            same = same and torch.equal(all_c[r * per * CB: r * per * CB + (rhi - rlo) * CB], ref_c[rlo * CB: rhi * CB])
        if not agree(same):
            raise SystemExit(f"bench.py: {key}: the sharded + gathered output differs from the one-GPU output")
        out[key] = {"total_blobs": total, "blobs_per_rank": per,
                    "one_gpu_ms": round(t_one * 1e3, 3), "one_gpu_blobs_per_s": round(total / t_one),
                    "sharded_ms_gather_proofs": round(t_p * 1e3, 3), "sharded_blobs_per_s_gather_proofs": round(total / t_p),
                    "sharded_ms_gather_cells_and_proofs": round(t_full * 1e3, 3), "sharded_blobs_per_s_gather_cells_and_proofs": round(total / t_full),
                    "speedup_over_one_gpu": round(t_one / t_p, 3), "gathered_equals_one_gpu_output": True,
                    "gather_bytes_per_rank": {"proofs": per * PB, "cells": per * CB}}
        del blobs_all, ref_c, ref_p, loc_c, loc_p, all_c, all_p, one_c, one_p
    out["note"] = ("strong scaling: fixed total split over the ranks; a pass = slice compute + all-gather, timed pass by pass (median "
                   "of 5, MAX over ranks). Expect well below N x: 64 blobs per GPU do not fill an MI355X (DESIGN.md section 6)")
    return out


def device_list_leg(kzg, devices, blobs_h, per_device, steps=3, ref_ctx=None):
    """ONE context over a device list behind the unchanged ABI (eth_kzg_amd_das_context_new_on_devices; a drop-in host sets
    ETH_KZG_AMD_DEVICES and keeps calling eth_kzg_das_context_new): a host-pointer batch of per_device x len(devices) blobs through
    eth_kzg_amd_compute_cells_and_kzg_proofs_batch -- contiguous slices, one host thread per device, the caller's buffers are the
    gather target, no collective -- timed as a host sees it (PCIe both ways, gather and scatter included).  ref_ctx: a one-device
    context whose bytes the first blob of every slice must equal.  Runs on the library's current table budget."""
    import numpy as np
    n = per_device * len(devices)
    reps = -(-n // blobs_h.shape[0])
    blobs = np.ascontiguousarray(np.concatenate([blobs_h] * reps)[:n]) if reps > 1 else np.ascontiguousarray(blobs_h[:n])
    t0 = time.perf_counter()
    ctx = kzg.DASContext(use_precomp=True, devices=list(devices))
    t_ctx = time.perf_counter() - t0
    try:
        bufs = ctx.host_batch_buffers(n)
        st = ctx.compute_cells_and_kzg_proofs_batch_np(blobs, bufs)
        assert list(st) == [0] * n, "device-list context: a synthetic blob was rejected"
        checked = None
        if ref_ctx is not None:
            checked = True
            for d in range(len(devices)):
                b = d * n // len(devices)
                rc, rp = ref_ctx.compute_cells_and_kzg_proofs(blobs[b].tobytes())
                checked = checked and bufs["cells"][b].tobytes() == b"".join(rc) and bufs["proofs"][b].tobytes() == b"".join(rp)
            if not checked:
                raise SystemExit("bench.py: the device-list context's output differs from the one-device context's")
        ts = []
        for _ in range(steps):
            t1 = time.perf_counter()
            ctx.compute_cells_and_kzg_proofs_batch_np(blobs, bufs)
            ts.append(time.perf_counter() - t1)
        return {"devices": ctx.devices(), "blobs": n, "blobs_per_s": round(n / _median(ts)), "ms_per_call": round(_median(ts) * 1e3, 2),
                "context_s": round(t_ctx, 2), "window_bits": ctx.window_bits(), "table_GB_all_devices": round(ctx.table_bytes() / 1e9, 1),
                "first_blob_of_every_slice_checked_against_one_device": checked,
                "entry": "eth_kzg_amd_compute_cells_and_kzg_proofs_batch on ONE context over the device list (single process, one host "
                         "thread per device, no collective); host pointers: PCIe both ways, gather and scatter included"}
    finally:
        ctx.close()


def kernel_sources_hash():
    """SHA-256 over the sources of the dominant kernel (the GLV MSM and the field / curve headers it is made of): the key that
    ties a committed PMC profile to the build it was collected on (tools/pmc_summary.py stores it, bench.py compares it)."""
    import hashlib
    h = hashlib.sha256()
    for f in ("k_msm_glv.inc", "k_msm_glv16.hip", "curve30.hpp", "fp30.hpp", "fp30_mac.hpp", "fp30_consts.hpp", "curve29.hpp", "fp29.hpp", "fp29_mac.hpp", "fp29_consts.hpp", "glv.hpp", "Makefile"):
        with open(os.path.join(ROOT, "rust-eth-kzg_amd", "csrc", f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()


DUMP_BLOBS = {"cells": 32, "proofs": 1024}  # --dump-outputs: at most this many blobs per array (32 MB + 24 MB as float32)
DUMP_SEED = 0x4B5A47


def dump_outputs(dirname, d_cells, d_proofs, B):
    """--dump-outputs DIR: what the last timed step handed its caller -- every blob's 128 cells and 128 proofs -- as
    DIR/cells.npy (blobs x 128 x 2048) and DIR/proofs.npy (blobs x 128 x 48), byte values in float32 (exact).  A batch larger
    than DUMP_BLOBS is sampled: the same seeded, sorted choice of blob indices for the same --blobs-per-gpu, every run."""
    import numpy as np
    import torch
    os.makedirs(dirname, exist_ok=True)
    for name, d, per_blob in (("cells", d_cells, CELLS * BYTES_PER_CELL), ("proofs", d_proofs, CELLS * 48)):
        k = DUMP_BLOBS[name]
        idx = np.arange(B) if B <= k else np.sort(np.random.RandomState(DUMP_SEED).choice(B, k, replace=False))
        rows = d.view(B, per_blob)[torch.from_numpy(idx).to(d.device)].cpu().numpy()
        np.save(os.path.join(dirname, name + ".npy"), rows.reshape(len(idx), CELLS, -1).astype(np.float32))


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _launch(n, argv):
    """`python bench.py --gpus N` with N > 1 and no launcher environment: start one rank per GPU as CHILD processes
    (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set as torch.distributed.run would) and relay rank 0's JSON line.  This
    parent never imports torch and never touches the GPU (no exec of a GPU-initialised process either: children are
    spawned, the parent waits and exits with the first non-zero child status)."""
    import threading
    port = int(os.environ.get("MASTER_PORT", "0")) or _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "KZG_BENCH_LAUNCHER": "bench.py"})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", "1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=sys.stderr))

    def relay():
        for line in procs[0].stdout:
            sys.stdout.write(line.decode(errors="replace"))
            sys.stdout.flush()
    th = threading.Thread(target=relay, daemon=True)
    th.start()
    rc, live = 0, set(range(n))
    while live:
        for r in sorted(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"bench.py: rank {r} exited with status {code}; stopping the other ranks", file=sys.stderr, flush=True)
                for o in live:  # exactly the children started above, by their own handles
                    procs[o].terminate()
        time.sleep(0.05)
    th.join(timeout=10)
    sys.exit(rc)


def _launcher_selftest(args):
    """No GPU: every rank reports the environment the launcher gave it, the ranks meet on a gloo rendezvous (barrier +
    all-gather), rank 0 prints one JSON line.  tests/test_bench_launcher.py runs this with --gpus 2."""
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    me = {"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", "0")), "world": world, "pid": os.getpid(),
          "master": os.environ.get("MASTER_ADDR", "") + ":" + os.environ.get("MASTER_PORT", ""),
          "launcher": os.environ.get("KZG_BENCH_LAUNCHER", "external")}
    ranks = [me]
    if world > 1:
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        dist.barrier()
        ranks = [None] * world
        dist.all_gather_object(ranks, me)
        dist.barrier()
        dist.destroy_process_group()
    if os.environ.get("KZG_BENCH_SELFTEST_FAIL_RANK") == str(rank):  # the test of the failure path
        sys.exit(7)
    watchdog = None
    if world > 1 and "KZG_BENCH_SELFTEST_HANG_RANK" in os.environ:
        # the test of the communicator-init watchdog, through the code bench.py itself runs (sharding.attach_library_comm): a
        # stand-in context whose comm_init never comes back on one rank -- every rank must be told so, none may wait for it
        sharding = importlib.import_module("rust-eth-kzg_amd.sharding")
        hang = int(os.environ["KZG_BENCH_SELFTEST_HANG_RANK"])

        class _StuckComm:
            destroyed = False

            def comm_probe(self):
                return "librccl (stand-in)"

            def comm_unique_id(self):
                return bytes(128)

            def comm_init(self, uid, r, w):
                if r == hang:
                    time.sleep(3600)

            def comm_info(self):
                return rank, world

            def comm_destroy(self):
                self.destroyed = True
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        fake = _StuckComm()
        t0 = time.perf_counter()
        ok = sharding.attach_library_comm(fake, dist)
        mine = {"rank": rank, "attached": ok, "stuck": bool(sharding.attach_library_comm.stuck), "waited_s": round(time.perf_counter() - t0, 2),
                "error": sharding.attach_library_comm.last_error, "destroyed": fake.destroyed}
        watchdog = [None] * world
        dist.all_gather_object(watchdog, mine)
        dist.barrier()
        dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"launcher_selftest": True, "n_gpus": world, "gpus_arg": args.gpus, "ranks": ranks, "watchdog": watchdog}), flush=True)
        sys.stdout.flush()
        os._exit(0)  # (the rank with the sleeping thread could not leave otherwise: what bench.py does after a real watchdog event)
    if rank == 0:
        print(json.dumps({"launcher_selftest": True, "n_gpus": world, "gpus_arg": args.gpus, "ranks": ranks}), flush=True)


def context_creation_times(ctx, t_ctx0, t_ctx_new, build_probe):
    """--full: context creation as the reference's "Initialize context" bench sees it (benchmark-mt.rs:103-113): the constructor
    returned on small start tables (progressive start) t_ctx_new after t_ctx0; a first result is computed on them, then the wide
    tables arrive.  Returns the figures once the wide tables are in use."""
    start_width = ctx.window_bits()
    first_blob = synth_blobs(1, seed=0x4B5A47)[0].tobytes()
    first_out = ctx.compute_cells_and_kzg_proofs(first_blob)
    t_ctx_first = time.perf_counter() - t_ctx0
    _mark("first result computed")
    # While the helper thread allocates (pieces of < 1 GB) and builds the wide tables, a caller keeps working: one
    # compute_cells_and_kzg_proofs through the reference's entry point every 5 ms.  How long the slowest of them took is the
    # stall a service sees during start-up (round 3: one 206 GB hipMalloc froze every HIP call of the process for 2-4.4 s).
    waits, wait_at, half_s = [], [], None
    while ctx.tables_ready(0) == 0 and build_probe:
        t1 = time.perf_counter()
        out_k = ctx.compute_cells_and_kzg_proofs(first_blob)
        waits.append(time.perf_counter() - t1)
        wait_at.append(t1 - t_ctx0)
        assert out_k == first_out, "a call made while the wide tables were being built returned different bytes"
        g = ctx.table_groups_ready()
        if half_s is None and (g >= 64 or ctx.window_bits() != start_width):
            half_s = time.perf_counter() - t_ctx0
        time.sleep(0.005)
    tables_state = ctx.tables_ready(-1)
    t_ctx = time.perf_counter() - t_ctx0
    _mark("wide tables ready")
    assert ctx.compute_cells_and_kzg_proofs(first_blob) == first_out, "start tables and wide tables disagree"
    ws = sorted(waits)
    return {"constructor_returns_s": round(t_ctx_new, 3), "first_result_s": round(t_ctx_first, 3), "wide_tables_in_use_s": round(t_ctx, 2),
            "half_of_the_fk20_groups_on_the_wide_table_s": round(half_s, 2) if half_s is not None else None,
            "start_table_window_bits": start_width, "final_state": tables_state,
            "table_allocation": dict(ctx.table_build_info(), note="hipMalloc of the wide tables' pieces (< 1 GB each). On an idle GPU a piece takes ~2 ms (206 GB: 0.4 s); "
                                     "a piece that takes seconds is the driver wiping memory another process has just freed, and this process's GPU queues "
                                     "stand still meanwhile -- that, not the library, is what the longest call during the build then shows"),
            "calls_during_build": {"calls": len(ws), "calls_per_s": round(len(ws) / max(1e-9, t_ctx - t_ctx_first), 1) if ws else None,
                                   "longest_ms": round(ws[-1] * 1e3, 2) if ws else None, "p99_ms": round(ws[int(0.99 * (len(ws) - 1))] * 1e3, 2) if ws else None,
                                   "median_ms": round(ws[len(ws) // 2] * 1e3, 2) if ws else None,
                                   "slowest_three_at_s_ms": [[round(a, 2), round(w * 1e3, 1)] for w, a in sorted(zip(waits, wait_at), reverse=True)[:3]],
                                   "what": "eth_kzg_compute_cells_and_kzg_proofs of one blob every 5 ms from the calling thread while the helper thread "
                                           "allocates and builds ~250 GB of window tables; bytes checked against the first result every time"}}


def roofline_figures(stages, steps, B, value, window_bits, linmap):
    """--full: the per-stage HIP-event times of the timed steps and the roofline views of their dominant kernel."""
    # dominant kernel = the one with the largest accumulated HIP-event time
    dom = max(stages, key=lambda s: stages[s][0])
    dom_ms, dom_launches = stages[dom]
    per_launch_s = dom_ms * 1e-3 / max(1, dom_launches)
    # gathered additions per (scalar, base) of the FK20 table IN USE: 2 ceil(128 / w) for a GLV table of width w (both 128-bit
    # halves over the same windows), ceil(255 / w) for a plain one
    msm_adds = 2 * -(-128 // window_bits)
    # algorithmic bytes per launch of each kernel family (DESIGN.md "kernels"):
    alg_bytes = {
        "blob_to_coeffs": B * (BYTES_PER_BLOB + 4096 * 32),
        "coeffs_to_cells": B * (4096 * 32 * 2 + 8192 * 32),
        "fk20_scalars": B * (4096 * 32 + 128 * 64 * 32),
        # scalars in + one 96-B table entry per (scalar, window) + 128 Jacobian sums out
        # (2 ceil(128 / w) packed 96-B entries per scalar: 16 at the widest table)
        "msm_fixed": B * (128 * 64 * 32 + 128 * 64 * msm_adds * 96 + 128 * 168),
        # one radix-2 layer: 64 butterflies x (2 points in, 2 points out) x 168 B per blob
        "g1_ifft": B * 64 * 4 * 168,
        "g1_fft": B * 64 * 4 * 168,
        "compress": B * 128 * (168 + 48),
        # compiled linear map: ~3.9 k point operations per blob (350 constant multiplications, 3.2 k additions, 0.4 k
        # doubling runs), each reading one or two 168-B points and writing one, over its ~42 launches
        "g1_linmap": B * (sum(linmap[:2]) + 400) * 3 * 168 // max(1, linmap[3]),
    }[dom]
    achieved = alg_bytes / per_launch_s / 1e9
    # HBM traffic of the dominant kernel: NOT measured in this run (PMC passes need rocprofv3) -- taken from the newest
    # committed profile of this round and labelled with its file name; valid only for the configuration it was collected on
    traffic, traffic_source, insts_valu, insts_source = None, None, None, None
    try:
        import glob
        files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9]*_pmc_b2048*.json")))
        pmc_doc = json.load(open(files[-1]))
        pm = pmc_doc["kernels"]
        # the counters are only quoted for the build they were collected on: the profile records a hash of the dominant
        # kernel's sources (tools/pmc_summary.py); a build whose sources differ gets traffic = null instead of stale numbers
        if pmc_doc.get("msm_kernel_sources_sha256") != kernel_sources_hash():
            raise RuntimeError("committed PMC profile belongs to another build of the kernel")
        want = {"msm_fixed": ("k_msm_glv_chunked",), "g1_linmap": ("k_slp_mulc",)}.get(dom, ())
        key = next((k for w_ in want for k in pm if w_ in k), None)  # the newest profile names the kernel the default schedule runs
        if key in pm and B == 2048 and window_bits == 16:
            # gfx950 correction (MI355X_MICROARCH.md, calibrated for this kernel's 16-B-per-lane gathers in
            # profiles/r1f_calib_fetch.log): FETCH_SIZE tallies every 128-B line request at 64 B -> double it; WRITE_SIZE is exact
            traffic = (2.0 * pm[key]["FETCH_SIZE_per_launch_max"] + pm[key]["WRITE_SIZE_per_launch_max"]) * 1024.0
            traffic_source = os.path.relpath(files[-1], ROOT) + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of an earlier run of this command; not re-measured here)"
            insts_valu = pm[key].get("SQ_INSTS_VALU_per_launch_max")
            insts_source = os.path.relpath(files[-1], ROOT) + " (SQ_INSTS_VALU of the same build, rocprofv3 --pmc)"
    except Exception:
        pass
    if insts_valu is None and dom == "msm_fixed":
        # no counter file for this build: the static count of the kernel's hot loop (4,066 VALU instructions per gathered addition in
        # the disassembly + the folds; 4,090 per addition measured by SQ_INSTS_VALU on round 5's build) x the additions of a launch
        insts_valu = 4090.0 * B * 128 * 64 * msm_adds / 64.0
        insts_source = "static count: 4,090 wave-instructions per gathered addition (profiles/r5c_pmc_sq_b2048_glv16.json) x additions per launch / 64 lanes"
    stage_ms_per_step = {s: round(stages[s][0] / steps, 3) for s in stages}
    # integer-VALU view (the bound that actually binds)
    mac_rate = value * 1.0e9 / 1e9  # reference-algorithm count: ~1.0e9 32x32 MACs per blob
    li = linmap
    mul_eq = fp_mul_eq_per_blob(window_bits, li[:3] if li[0] else (642, 14 * 64 * 1.5, 0), B)
    mul_rate = value * mul_eq / 1e9
    return {
        # What binds the dominant kernel is integer-VALU issue: achieved = wave-instructions x 64 lanes
        # / launch time, peak = the measured issue ceiling of this kernel's own 12 : 4 multiply-add mix at the two waves per SIMD its
        # 212 registers allow (34.4 T lane-ops/s at 2.4 GHz, profiles/r3_ubench_issue.log).  NOTE: under this kernel the chip does
        # not hold 2.4 GHz -- the SMI reports ~2.0-2.1 GHz at ~1.27 kW (profiles/r5c_bench_clocks_power.log) -- so frac < 1 is mostly
        # clock, not idle issue slots: GRBM_GUI_ACTIVE / launch time gives the clock, SQ_INSTS_VALU / GRBM cycles the issue rate.
        "roofline": {"bound": "valu-int", "kernel": dom,
                     "achieved": (insts_valu * 64.0 / per_launch_s / 1e12) if insts_valu else None, "peak": VALU_MIX_PEAK_TLOPS, "unit": "T lane-ops/s",
                     "frac": (insts_valu * 64.0 / per_launch_s / 1e12 / VALU_MIX_PEAK_TLOPS) if insts_valu else None,
                     "wave_instructions_per_launch": insts_valu, "instructions_source": insts_source,
                     "traffic": traffic, "traffic_source": traffic_source,
                     "avg_launch_ms": per_launch_s * 1e3, "launches_per_step": dom_launches // max(1, steps),
                     "note": "integer-VALU issue is what binds (MFMA unused: no dense contraction); peak = measured issue ceiling of the kernel's "
                             "multiply-add mix at 2 waves/SIMD and 2.4 GHz; the kernel runs at ~2.0-2.1 GHz (power), see roofline_hbm for the byte view"},
        # the HBM view the contract names, kept as the secondary: both byte counts side by side -- the MANDATORY bytes of SURVEY 8(d)
        # for this kernel (scalars in + sums out) and the bytes the design chooses to gather from its window table
        "roofline_hbm": {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "algorithmic_bytes_per_launch_gathered": alg_bytes,
                         "algorithmic_bytes_per_launch_mandatory": B * (128 * 64 * 32 + 128 * 168) if dom == "msm_fixed" else alg_bytes,
                         "frac_mandatory": (B * (128 * 64 * 32 + 128 * 168) if dom == "msm_fixed" else alg_bytes) / per_launch_s / 1e9 / HBM_PEAK_GBS,
                         "whole_path_mandatory_bytes_per_blob": ALG_BYTES_PER_BLOB,
                         "traffic": traffic, "traffic_source": traffic_source},
        "roofline_valu": {"bound": "valu-int", "achieved": mul_rate, "peak": FP_MUL_PEAK_G, "unit": "G Fp-mul/s",
                          "frac": mul_rate / FP_MUL_PEAK_G, "fp_mul_eq_per_blob": round(mul_eq),
                          "reference_algorithm_mac_rate_G": mac_rate, "mac_issue_peak_G": VALU_INT_PEAK_GOPS,
                          "note": "blobs/s x Fp-multiplication equivalents this build executes per blob / measured sustained "
                                  "multiplication rate of the signed 13 x 30-bit field (tools/ubench_fp30 --sustained, 2 waves/SIMD); "
                                  "reference_algorithm_mac_rate = blobs/s x 1.0e9 MACs (SURVEY 8d)"},
        "whole_path_hbm_frac": value * ALG_BYTES_PER_BLOB / 1e9 / HBM_PEAK_GBS,
        "stage_ms_per_step": stage_ms_per_step,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--blobs-per-gpu", type=int, default=int(os.environ.get("KZG_BENCH_BLOBS", "2048")))
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the correctness gate, context-creation figures, per-stage times and roofline, the "
                         "timing without stage events, the single-blob latency, the CPU baseline and the side configurations (N = 1), "
                         "the exchange check and the strong-scaling and device-list legs (N > 1); the --no-* options below drop single legs")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the last step's cells and proofs as DIR/<name>.npy (float32; see dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-configs", action="store_true", help="skip the side configurations (BASELINE configs 3-5, ABI, context creation)")
    ap.add_argument("--no-latency-probe", action="store_true",
                    help="skip the 1-blob latency launches (profiling runs: keeps rocprofv3's per-kernel averages to full-batch launches)")
    ap.add_argument("--no-build-probe", action="store_true",
                    help="do not issue single-blob calls while the wide tables are built (profiling runs: keeps those launches, slowed by the "
                         "table builder next to them, out of rocprofv3's per-kernel averages)")
    ap.add_argument("--strong-configs", action="store_true",
                    help="with --full: also run the strong-scaling legs (configs 4 and 5 as written) at N = 1; a --full run at N > 1 always has them")
    ap.add_argument("--launcher-selftest", action="store_true", help="CPU only: check the --gpus N launcher and the rendezvous, then exit")
    ap.add_argument("--no-device-list-leg", action="store_true",
                    help="skip the single-process leg: ONE context over the device list (N > 1: all N GPUs from rank 0 after the ranks "
                         "have freed theirs; N = 1: the list 0,0 on the default tables) beside the process-per-GPU form")
    ap.add_argument("--table-sharding", choices=["blob"], default="blob",
                    help="how the FK20 work is cut over GPUs: by blob (every GPU holds every group's table; the only form built -- the "
                         "group-sharded 19-bit-window design of DESIGN.md section 6 is priced there and not implemented)")
    ap.add_argument("--exchange", choices=["library", "library-required", "torch"], default="library",
                    help="N > 1: the all-gather runs on the library's own RCCL communicator (default; if it cannot be built the run goes "
                         "on over torch.distributed's and SAYS SO in config.exchange and on stderr; library-required: fail instead), "
                         "or on torch.distributed's by choice")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.strong_configs and not args.full:
        ap.error("--strong-configs is a leg of a --full run")

    # --gpus N is authoritative: without a launcher's environment bench.py starts the N ranks itself -- before torch or
    # the GPU is touched in this process
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _launch(args.gpus, sys.argv[1:])
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher environment says WORLD_SIZE={world}")
    if args.launcher_selftest:
        return _launcher_selftest(args)

    # stdout carries exactly ONE line, the JSON record: native libraries write banners to the C-level stdout (RCCL prints its
    # version block there when a communicator is built, flushed at exit, i.e. after the record), so file descriptor 1 is
    # pointed at stderr for the rest of the process and the record goes out through a private copy of the real stdout
    sys.stdout.flush()
    record_fd = os.dup(1)
    os.dup2(2, 1)

    rccl_log = None
    if world > 1:  # RCCL's own warnings go to a file per rank, so that a failed communicator can be explained in the record
        rccl_log = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"kzg_bench_rccl_rank{rank}_{os.getpid()}.log")
        os.environ.setdefault("NCCL_DEBUG", "WARN")
        os.environ.setdefault("NCCL_DEBUG_FILE", rccl_log)
    import torch
    import torch.distributed as dist

    rehearsal = world > 1 and os.environ.get("KZG_BENCH_REHEARSAL") == "1"
    if rehearsal:  # N ranks on GPU 0 (see _Harness): small tables so that N contexts fit, torch's gloo for the harness collectives
        local_rank = 0
        os.environ.setdefault("ETH_KZG_AMD_TABLE_GB", "24")
    # The library's default table budget is a stated 108 GB (nine-window GLV tables for FK20 and for commitments); the bench measures the path at the widest tables the GPU
    # holds and says so in config.table_budget (blobs_per_s_vs_table_memory carries the default's and every other size's rate)
    os.environ.setdefault("ETH_KZG_AMD_TABLE_GB", "max")
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit(f"bench.py: rank {rank} needs GPU {local_rank} but only {torch.cuda.device_count()} are visible "
                         f"(--gpus {args.gpus})")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo" if rehearsal else "nccl", rank=rank, world_size=world)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    kzg = importlib.import_module("rust-eth-kzg_amd")
    sharding = importlib.import_module("rust-eth-kzg_amd.sharding")
    # The constructor returns on small start tables (progressive start) while a helper thread builds the wide ones; --full
    # times that start-up as a caller sees it (context_creation_times), a plain run just waits for the wide tables.
    ctx_times = None
    t_ctx0 = time.perf_counter()
    ctx = kzg.DASContext(use_precomp=True, device=local_rank, wait_tables=False)  # no CPU fallback: raises/aborts without the HIP path
    t_ctx_new = time.perf_counter() - t_ctx0
    _mark("context constructed")
    if args.full:
        ctx_times = context_creation_times(ctx, t_ctx0, t_ctx_new, build_probe=not args.no_build_probe)
    else:
        ctx.tables_ready(-1)  # the headline runs on the wide tables
        _mark("wide tables ready")

    B = args.blobs_per_gpu
    blobs_h = synth_blobs(B, seed=0x4B5A47 + rank)
    d_blobs = torch.from_numpy(blobs_h).to(dev)
    d_cells = torch.empty(B * CELLS * BYTES_PER_CELL, dtype=torch.uint8, device=dev)
    d_proofs = torch.empty(B * CELLS * 48, dtype=torch.uint8, device=dev)
    d_all_proofs = torch.empty(world * B * CELLS * 48, dtype=torch.uint8, device=dev) if world > 1 else None
    stream = torch.cuda.Stream(device=dev)  # a real (non-null) HIP stream: kernels are enqueued on it without host syncs
    hz = _Harness(torch, dist, dev, rehearsal)
    # the exchange runs on the library's own RCCL communicator (what a C / Go / Java host would use); torch.distributed
    # carries the 128-byte id and stays the fallback if the library cannot build its communicator
    lib_comm, comm_ranks, rccl_file, comm_error = False, None, None, None
    if world > 1 and args.exchange in ("library", "library-required"):
        try:
            rccl_file = ctx.comm_probe()  # which librccl file the library bound (torch's already-mapped copy when present)
        except Exception:
            rccl_file = None  # attach_library_comm below reports the reason on every rank
        try:
            # all ranks or none (the ranks agree before anyone enters the collective ncclCommInitRank); raises with the reason on every rank
            lib_comm = sharding.attach_library_comm(ctx, dist, required=True)
            comm_ranks = ctx.comm_info()[1]
        except RuntimeError as e:
            if args.exchange == "library-required":
                raise
            comm_error = str(e)  # never silent: stderr now, config.exchange / config.library_communicator_error in the record
            try:  # what RCCL itself had to say (NCCL_DEBUG=WARN into NCCL_DEBUG_FILE, set above)
                with open(os.environ.get("NCCL_DEBUG_FILE", rccl_log or ""), "r", errors="replace") as fh:
                    tail = fh.read()[-1500:].strip()
                if tail:
                    comm_error += " | RCCL log: " + " / ".join(tail.splitlines()[-8:])
            except OSError:
                pass
            if rank == 0:
                print(f"bench.py: the library's RCCL communicator is unavailable ({comm_error}); the all-gather runs on torch.distributed's",
                      file=sys.stderr, flush=True)
    elif world == 1 and args.strong_configs and args.exchange != "torch":  # one-GPU box: the same calls on a 1-rank communicator
        rccl_file = ctx.comm_probe()
        ctx.comm_init(ctx.comm_unique_id(), 0, 1)
        lib_comm, comm_ranks = True, ctx.comm_info()[1]

    def step():
        with torch.cuda.stream(stream):
            ctx.compute_cells_and_kzg_proofs_device(B, d_blobs.data_ptr(), d_cells.data_ptr(), d_proofs.data_ptr(),
                                                    want_status=False, stream=stream.cuda_stream)
            if world > 1:  # the only exchange: proof vectors over RCCL/xGMI
                if lib_comm:
                    sharding.all_gather_proofs(ctx, d_proofs, d_all_proofs, stream)
                else:
                    hz.all_gather_into(d_all_proofs, d_proofs)

    def fence():
        torch.cuda.synchronize(dev)
        t_local = time.perf_counter()  # this rank's own work is done here, before it waits for the others
        if world > 1:
            hz.barrier()
        torch.cuda.synchronize(dev)
        return t_local

    gather_checked = None
    if args.full:
        # correctness gate on the first run (status + the data-in-first-half invariant, fk20/prover.rs:251-275)
        st = ctx.compute_cells_and_kzg_proofs_device(B, d_blobs.data_ptr(), d_cells.data_ptr(), d_proofs.data_ptr(),
                                                     want_status=True, stream=None)
        assert st == [0] * B, "synthetic blobs rejected"
        torch.cuda.synchronize(dev)
        first_half = d_cells.view(B, 2, 64 * BYTES_PER_CELL)[:, 0, :]
        assert torch.equal(first_half, d_blobs), "cells[0..63] != blob"

        if world > 1:  # the exchange itself, once, before timing: rank r's slab of the gathered vector must be rank r's proofs
            step()
            fence()
            mine = d_proofs.view(-1, 8).view(torch.int64).sum().reshape(1)
            sums = torch.empty(world, dtype=torch.int64, device=dev)
            hz.all_gather_into(sums, mine)  # (torch's communicator: an independent path for the check)
            got = d_all_proofs.view(world, -1, 8).view(torch.int64).sum(dim=(1, 2))
            gather_checked = bool(torch.equal(sums, got)) and bool(torch.equal(d_all_proofs.view(world, -1)[rank], d_proofs))
            flag = torch.tensor([1 if gather_checked else 0], dtype=torch.int32, device=dev)
            hz.all_reduce(flag, dist.ReduceOp.MIN)
            if not int(flag.item()):
                raise SystemExit("bench.py: the all-gathered proof vector does not match the ranks' own proofs")
        _mark("correctness gate passed")
    _mark("warm-up")
    for _ in range(args.warmup):
        step()
    fence()
    # the timed region, the same in a plain and a --full run (with the per-stage events it has always had, so that ms_per_step
    # keeps its meaning; --full reports the stage times and the cost of the events)
    ctx.set_profiling(True)
    ctx.get_stage_times()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    t_local_end = fence()
    dt = time.perf_counter() - t0
    stages = ctx.get_stage_times()
    ctx.set_profiling(False)
    _mark("timed steps done")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, d_cells, d_proofs, B)
    dt_rank = t_local_end - t0  # without the wait for the slowest rank
    per_rank_ms, gather_ms = None, None
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        hz.all_reduce(t, dist.ReduceOp.MAX)
        dt = float(t.item())
    if world > 1 and args.full:
        # one line must be enough to diagnose a bad scaling curve: every rank's own time per step, and the all-gather alone
        mine = torch.tensor([dt_rank / args.steps * 1e3], dtype=torch.float64, device=dev)
        allr = torch.empty(world, dtype=torch.float64, device=dev)
        hz.all_gather_into(allr, mine)
        per_rank_ms = [round(float(v), 3) for v in allr.cpu()]
        fence()
        tg = time.perf_counter()
        for _ in range(args.steps):
            with torch.cuda.stream(stream):
                if lib_comm:
                    sharding.all_gather_proofs(ctx, d_proofs, d_all_proofs, stream)
                else:
                    hz.all_gather_into(d_all_proofs, d_proofs)
        fence()
        tgm = torch.tensor([(time.perf_counter() - tg) / args.steps * 1e3], dtype=torch.float64, device=dev)
        hz.all_reduce(tgm, dist.ReduceOp.MAX)
        gather_ms = round(float(tgm.item()), 3)
    dt_plain, lat = None, []
    if args.full:
        # the same K steps once more WITHOUT the per-stage events (they also keep the small-batch cells kernel on the main stream):
        # what the instrumentation of the timed region costs, stated instead of assumed
        fence()
        t0u = time.perf_counter()
        for _ in range(args.steps):
            step()
        fence()
        dt_plain = time.perf_counter() - t0u
        if world > 1:
            t = torch.tensor([dt_plain], dtype=torch.float64, device=dev)
            hz.all_reduce(t, dist.ReduceOp.MAX)
            dt_plain = float(t.item())

        # single-blob latency (BASELINE.json config 2), outside the timed region
        for _ in range(0 if args.no_latency_probe else 3):
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            with torch.cuda.stream(stream):
                ctx.compute_cells_and_kzg_proofs_device(1, d_blobs.data_ptr(), d_cells.data_ptr(), d_proofs.data_ptr(),
                                                        want_status=False, stream=stream.cuda_stream)
            torch.cuda.synchronize(dev)
            lat.append(time.perf_counter() - t1)

    strong = None
    if args.full and (world > 1 or args.strong_configs):
        try:
            strong = strong_configs(ctx, sharding, torch, dist, dev, world, rank, lib_comm, stream, hz)
        except SystemExit:
            raise  # a parity failure of the gathered output must sink the run
        except Exception as e:  # anything else in the side legs must not cost the headline record
            strong = {"error": repr(e)}

    # what the record quotes from the context (read now: at N > 1 the context is freed before the record is written)
    ctx_window_bits, ctx_table_bytes, ctx_linmap = ctx.window_bits(), ctx.table_bytes(), ctx.linmap_info()
    device_list = None
    if world > 1 and args.full and not args.no_device_list_leg:
        # The process-per-GPU form is measured; now the form a drop-in host gets without launching anything: rank 0 alone, ONE context
        # over all N GPUs.  Every rank first frees its context (its tables would not leave room for a second set on its GPU), the
        # others wait at the barrier.  On the library's DEFAULT table budget (what such a host gets), per-GPU share = half the
        # headline's (host memory: 0.4 MB per blob).  A failure here costs this leg, never the record.
        saved_budget = os.environ.get("ETH_KZG_AMD_TABLE_GB")
        try:
            if lib_comm:
                ctx.comm_destroy()
            ctx.close()
            ctx = None
            hz.barrier()
            if rank == 0:
                if rehearsal:
                    os.environ["ETH_KZG_AMD_TABLE_GB"] = "24"
                else:
                    os.environ.pop("ETH_KZG_AMD_TABLE_GB", None)
                devs = [0] * world if rehearsal else list(range(world))
                device_list = device_list_leg(kzg, devs, blobs_h, per_device=max(1, min(B, 1024)), steps=3)
        except SystemExit:
            raise
        except Exception as e:  # noqa: BLE001
            device_list = {"error": repr(e)}
        finally:
            if saved_budget is None:
                os.environ.pop("ETH_KZG_AMD_TABLE_GB", None)
            else:
                os.environ["ETH_KZG_AMD_TABLE_GB"] = saved_budget
            hz.barrier()

    if rank == 0:
        total_blobs = B * world * args.steps
        value = total_blobs / dt
        wbits = ctx_window_bits
        msm_adds = 2 * -(-128 // wbits)  # gathered additions per (scalar, base) of the FK20 table in use
        li = ctx_linmap
        out = {
            "metric": "blobs/sec compute_cells_and_kzg_proofs (4096-pt blob)",
            "value": value, "unit": "blobs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u32", "dtype_note": "381-bit Fp as 13 signed 30-bit digits (everything between the scalars and the proof bytes of this batch: MSM, the G1 linear map's multiplications and additions), 14x29-bit / 12x32-bit limbs in the latency paths, codecs and verification, 255-bit Fr as 8x32-bit (stored) and 9x29-bit (inside the transforms) limbs, Montgomery integers; exact arithmetic", "data": "synthetic",
            "config": {"workload": f"compute_cells_and_kzg_proofs on DEVICE-RESIDENT blobs (inputs and outputs stay in HBM; the "
                                   f"host-pointer ABI rate is configs.abi_host_pointer_batch), batch-saturated: {B} synthetic blobs "
                                   f"per GPU per step (config 2's single blob: single_blob_latency_ms of a --full run)",
                       "blobs_per_gpu": B, "use_precomp": True, "window_bits": ctx_window_bits,
                       "fk20_table": f"GLV: {msm_adds // 2} windows of {wbits} bits per 128-bit half scalar, packed 96-B entries, {msm_adds} gathered additions per base",
                       "table_GB": round(ctx_table_bytes / 1e9, 2),
                       "table_budget": "ETH_KZG_AMD_TABLE_GB=" + os.environ.get("ETH_KZG_AMD_TABLE_GB", "") + " (set by bench.py: the widest tables the HBM holds; "
                                       "the library's default budget is 108 GB = nine-window GLV tables, see configs.blobs_per_s_vs_table_memory)",
                       "g1_transforms": f"compiled linear map: {li[0]} constant multiplications, {li[1]} additions, {li[2]} doublings per blob, {li[3]} launches" if li[0] else "radix-2 network",
                       "exchange": ("ncclAllGather of the proof vectors per step inside libc_eth_kzg.so (eth_kzg_amd_all_gather)" if lib_comm
                                    else "RCCL all-gather of proofs per step (torch.distributed)" + (" -- the library communicator FAILED: " + comm_error if comm_error else "")) if world > 1 else "none",
                       "library_communicator_error": comm_error,
                       "ranks": world, "library_communicator_ranks": comm_ranks, "rccl_library": rccl_file,
                       "launcher": os.environ.get("KZG_BENCH_LAUNCHER", "external (torch.distributed.run)") if world > 1 else "none",
                       "rehearsal": "KZG_BENCH_REHEARSAL=1: all ranks share GPU 0, gloo for the harness, small tables -- a check of the N > 1 code paths, NOT a measurement" if rehearsal else None,
                       "gathered_proofs_checked": gather_checked},
        }
        if args.full:
            out.update(roofline_figures(stages, args.steps, B, value, ctx_window_bits, ctx_linmap))
            out.update({"ms_per_step_without_stage_events": round(dt_plain / args.steps * 1e3, 3),
                        "ms_per_step_per_rank": per_rank_ms, "all_gather_ms_per_step": gather_ms,
                        "single_blob_latency_ms": (min(lat) * 1e3) if lat else None, "context_creation_s": None})
        if strong is not None:
            out["configs_strong"] = strong
        if device_list is not None:
            out["single_process_device_list"] = device_list
        if world > 1 and args.full:
            out["omitted_at_n_gpus_above_1"] = ["cpu_baseline", "configs (single-GPU side figures)", "blobs_per_s_vs_table_memory"]
        side = args.full and world == 1  # the single-GPU side figures of a --full run
        extra = None
        if side and not args.no_configs:
            out["configs"], extra = side_configs(ctx, kzg, torch, dev, blobs_h, ctx_times)
        if args.full:
            out["context_creation_s"] = ctx_times
        if side and not args.no_cpu_baseline:
            gpu_first = (bytes(d_cells[:CELLS * BYTES_PER_CELL].cpu().numpy()), bytes(d_proofs[:CELLS * 48].cpu().numpy()))
            out["cpu_baseline"] = cpu_baseline([bytes(blobs_h[i].tobytes()) for i in range(min(B, 32))], gpu_first=gpu_first, extra=extra)
            out["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
        if side and not args.no_configs:
            # blobs/s against window-table memory: the main context goes first (its 249 GB leave no room),
            # then one context per table size on the same resident batch.  UsePrecomp::Yes{width} is the reference's knob
            # (fixed_base_msm.rs:41-49).
            curve = [{"table": f"GLV width {ctx.window_bits()} for FK20 (eight windows of 16 bits) + nine windows for commitments (ETH_KZG_AMD_TABLE_GB=max)", "table_GB": round(ctx.table_bytes() / 1e9, 1),
                      "gathered_additions_per_base": 2 * -(-128 // ctx.window_bits()),
                      "blobs_per_s": round(value), "ms_per_step": round(dt / args.steps * 1e3, 2)}]
            ctx.close()
            ctx = None
            _mark("table curve")
            for label, env, precomp in (("nine GLV windows for FK20 and for commitments (ETH_KZG_AMD_TABLE_GB=108: the library's default budget)", {"ETH_KZG_AMD_TABLE_GB": "108"}, True),
                                        ("ten windows each (ETH_KZG_AMD_TABLE_GB=44)", {"ETH_KZG_AMD_TABLE_GB": "44"}, True),
                                        ("eleven windows each (ETH_KZG_AMD_TABLE_GB=22)", {"ETH_KZG_AMD_TABLE_GB": "22"}, True),
                                        ("sixteen windows each (use_precomp = false; also the tables every context starts on)", {}, False)):
                saved_env = {k: os.environ.get(k) for k in env}
                try:
                    _mark("table curve: " + label)
                    os.environ.update(env)
                    c2 = kzg.DASContext(use_precomp=precomp, device=local_rank)
                    ts = []
                    for it in range(4):
                        torch.cuda.synchronize(dev)
                        t0 = time.perf_counter()
                        with torch.cuda.stream(stream):
                            c2.compute_cells_and_kzg_proofs_device(B, d_blobs.data_ptr(), d_cells.data_ptr(), d_proofs.data_ptr(), want_status=False, stream=stream.cuda_stream)
                        torch.cuda.synchronize(dev)
                        if it >= 1:
                            ts.append(time.perf_counter() - t0)
                    if env.get("ETH_KZG_AMD_TABLE_GB") == "108" and not args.no_device_list_leg:
                        # beside the one-device context on the library's default tables: ONE context over the device list 0,0 (two
                        # engines on this GPU sharing its tables -- the code path of two GPUs on the one there is) and the same
                        # host-pointer batch on the one-device context, so that the pair can be compared
                        try:
                            _mark("device-list context 0,0 on the default tables")
                            hb = c2.host_batch_buffers(B)
                            c2.compute_cells_and_kzg_proofs_batch_np(blobs_h, hb)
                            th = []
                            for _ in range(3):
                                t0 = time.perf_counter()
                                c2.compute_cells_and_kzg_proofs_batch_np(blobs_h, hb)
                                th.append(time.perf_counter() - t0)
                            del hb
                            leg = device_list_leg(kzg, [local_rank, local_rank], blobs_h, per_device=B // 2, steps=3, ref_ctx=c2)
                            leg["same_batch_on_the_one_device_context_blobs_per_s"] = round(B / _median(th))
                            leg["note"] = "two engines on ONE GPU: a check of the device-list path and its cost, not a speed-up (the engines share the GPU)"
                            out["configs"]["device_list_context_0_0_default_tables"] = leg
                        except SystemExit:
                            raise
                        except Exception as e:  # noqa: BLE001
                            out["configs"]["device_list_context_0_0_default_tables"] = {"error": repr(e)}
                    w = c2.window_bits()
                    curve.append({"table": label, "table_GB": round(c2.table_bytes() / 1e9, 1),
                                  "gathered_additions_per_base": 2 * -(-128 // w),
                                  "blobs_per_s": round(B / _median(ts)), "ms_per_step": round(_median(ts) * 1e3, 2)})
                    c2.close()
                except Exception as e:
                    curve.append({"table": label, "error": repr(e)})
                finally:
                    for k, v in saved_env.items():
                        if v is None:
                            os.environ.pop(k, None)
                        else:
                            os.environ[k] = v
            out["configs"]["blobs_per_s_vs_table_memory"] = {"batch": B, "note": "table_GB = FK20 table + commitment table (both GLV tables; the commitment table has half the groups, and at most nine windows: 35 GB); same resident batch, median of 3 steps", "points": curve}
        os.write(record_fd, (json.dumps(out) + "\n").encode())
    if world > 1 and getattr(sharding.attach_library_comm, "stuck", False):
        # a thread of this rank is still inside ncclCommInitRank (the watchdog gave up on it): the record is out, leave without
        # running destructors that would wait for it
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
    if world > 1:
        dist.destroy_process_group()
    if ctx is not None:
        ctx.close()


if __name__ == "__main__":
    main()
