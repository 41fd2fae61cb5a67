// EIP-4844 single-point operations on the same kernels (first "next" row).
// Reference: crates/eip4844/src/prover.rs:32-88 (compute_kzg_proof, compute_blob_kzg_proof),
// crates/eip4844/src/verifier.rs:18-262 (verify_kzg_proof, verify_blob_kzg_proof, verify_blob_kzg_proof_batch and the
// two Fiat-Shamir transcripts), crates/cryptography/kzg_single_open/src/{prover.rs:33-65, verifier.rs:33-108}.
// GPU: blob -> coefficients (k_blob_to_coeffs), quotient by (X - z) (k_quotient_by_linear), MSM against the
// monomial SRS window table, decompression with subgroup checks, bucket MSMs of the verification equation.
// Host: SHA-256 transcripts, the handful of Fr products of the batch weights, the 2-pairing check.
#include "engine_internal.hpp"
#include "host_pairing.hpp"

namespace kzg {

// The device-resident core of every opening: blobs and Montgomery z_i in HBM -> y_i canonical and, if asked for, proof_i =
// commit(quotient_i), left on the device; per-blob status words in d_status_ (non-zero: a non-canonical element).
void Engine::open_blobs_core(int n, const uint8_t* d_blobs, const void* d_z_mont, void* d_y, uint8_t* d_proofs, hipStream_t st) {
    const int bp = ((n + 63) / 64) * 64;
    HIPCK(hipMemsetAsync(d_status_, 0, n * sizeof(int), st));
    launch::blob_to_coeffs(n, d_blobs, d_coeffs_, nullptr, d_status_, d_w29_, n_inv4096_, st);
    launch::quotient_by_linear(n, d_coeffs_, d_z_mont, d_canon_, d_y, st);
    if (d_proofs) {
        // proof = g1_lincomb(g1s[..4095], quotient) (kzg_single_open/src/prover.rs:40-43): the commitment MSM path
        launch::g1_set_inf(d_X_, (size_t)64 * bp, st, launch::FMT_JACS);
        launch_msm(d_canon_, TAB_SRS, d_X_, 64, n, bp, 0, st, launch::FMT_JACS);
        launch::g1_sum_positions(d_X_, 64, bp, n, st);
        launch::g1_compress(d_X_, d_proofs, 1, bp, n, st, launch::FMT_JACS);
    }
}

// blobs -> (status, y_i canonical, optionally proof_i = commit(quotient_i)); z_i Montgomery.  The upload step in front of the core
// and the download behind it: shared by compute_kzg_proof / compute_blob_kzg_proof (want_proofs) and the blob verifiers (y only).
int Engine::open_blobs_at(int n, const uint8_t* const* blobs, const Fr8* z_mont, bool want_proofs, uint8_t* h_proofs,
                          Fr8* h_y_canon, int* h_status) {
    hipStream_t st = stream_;
    ensure_workspace(n);
    PoolBuf d_blobs(*this, (size_t)n * BYTES_PER_BLOB), d_z(*this, (size_t)n * 32), d_y(*this, (size_t)n * 32), d_pr(*this, (size_t)n * 48);
    for (int b = 0; b < n; b++)
        HIPCK(hipMemcpyAsync((uint8_t*)d_blobs.p + (size_t)b * BYTES_PER_BLOB, blobs[b], BYTES_PER_BLOB, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(d_z.p, z_mont, (size_t)n * 32, hipMemcpyHostToDevice, st));
    open_blobs_core(n, (const uint8_t*)d_blobs.p, d_z.p, d_y.p, want_proofs ? (uint8_t*)d_pr.p : nullptr, st);
    if (want_proofs) HIPCK(hipMemcpyAsync(h_proofs, d_pr.p, (size_t)n * 48, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(h_y_canon, d_y.p, (size_t)n * 32, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(h_status, d_status_, n * sizeof(int), hipMemcpyDeviceToHost, st));
    SYNC_CHECKED(st);
    return OK;
}

int Engine::compute_kzg_proof_host(const uint8_t* blob, const uint8_t* z_bytes, uint8_t* out_proof, uint8_t* out_y) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        Fr z;
        bool z_ok = fr_from_be_canonical(z, z_bytes);
        if (!z_ok) z = zero<FrParams>();
        Fr8 z8 = to8(z), y8;
        int st = 0;
        uint8_t proof[48];
        const uint8_t* bl[1] = {blob};
        open_blobs_at(1, bl, &z8, true, proof, &y8, &st);
        if (st || !z_ok) return ERR_SCALAR;  // blob elements are checked first in the reference, then z
        memcpy(out_proof, proof, 48);
        fr_to_be(out_y, from8(y8));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// decompress + subgroup-check a few points on the GPU; returns per-point status
static void check_points(Engine* eng, const uint8_t* bytes, int n, void* d_out_affine, int* h_status, hipStream_t st, const Fp12w& beta) {
    PoolBuf d_b(*eng, (size_t)n * 48), d_st(*eng, (size_t)n * sizeof(int));
    HIPCK(hipMemcpyAsync(d_b.p, bytes, (size_t)n * 48, hipMemcpyHostToDevice, st));
    launch::g1_decompress((const uint8_t*)d_b.p, d_out_affine, (int*)d_st.p, n, 1, beta, st);
    HIPCK(hipMemcpyAsync(h_status, d_st.p, n * sizeof(int), hipMemcpyDeviceToHost, st));
    SYNC_CHECKED(st);

}

int Engine::compute_blob_kzg_proof_host(const uint8_t* blob, const uint8_t* commitment, uint8_t* out_proof) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        Fr z = blob_challenge(blob, commitment);
        Fr8 z8 = to8(z), y8;
        int st = 0, cst = 0;
        uint8_t proof[48];
        const uint8_t* bl[1] = {blob};
        open_blobs_at(1, bl, &z8, true, proof, &y8, &st);
        if (st) return ERR_SCALAR;
        PoolBuf d_pt(*this, sizeof(G1Affine));
        check_points(this, commitment, 1, d_pt.p, &cst, stream_, beta_);  // only validated (prover.rs:73-75)
        if (cst) return ERR_G1;
        memcpy(out_proof, proof, 48);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// e(sum_i a_i P_i, -[1]_2) * e(sum_i b_i Q_i, [tau]_2) == 1 with the two sums done as bucket MSMs on the GPU.
// d_points: [n_total] affine (job 0 = first n0 with sc0, job 1 = all n1 with sc1).  Returns 1 / 0.
int Engine::pairing_check_4844(const void* d_points, const std::vector<Fr8>& sc0, const std::vector<Fr8>& sc1, G1Affine* sums2) {
    hipStream_t st = stream_;
    const int n0 = (int)sc0.size(), n1 = (int)sc1.size();
    PoolBuf d_s0(*this, (size_t)n0 * 32), d_s1(*this, (size_t)n1 * 32), d_ws(*this, launch::pip_workspace_bytes(n1 > n0 ? n1 : n0)), d_out(*this, 2 * sizeof(G1Affine));
    HIPCK(hipMemcpyAsync(d_s0.p, sc0.data(), (size_t)n0 * 32, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(d_s1.p, sc1.data(), (size_t)n1 * 32, hipMemcpyHostToDevice, st));
    launch::msm_pippenger2(d_points, d_s0.p, n0, d_s1.p, n1, d_ws.p, d_out.p, beta_, st);
    G1Affine out[2];
    HIPCK(hipMemcpyAsync(out, d_out.p, sizeof out, hipMemcpyDeviceToHost, st));
    SYNC_CHECKED(st);
    // out[0] = rhs (pairs with [tau]_2), out[1] = lhs (pairs with -[1]_2)
    if (sums2) { sums2[0] = out[0]; sums2[1] = out[1]; }
    const pairing::G2Prepared* q[2] = {g2_tau1_.get(), g2_neg_gen_.get()};
    return pairing::product_is_one(out, q, 2) ? 1 : 0;
}


// TrustedSetup::check_powers: subgroup tests pass for a well-formed file in the wrong basis or order (Lagrange points handed in
// as monomial ones; two entries swapped) and every proof made on it is then wrong.  Both chains are checked to be consecutive
// powers of ONE tau with random 128-bit weights rho_i derived from the setup's bytes:
//   e(sum_i rho_i g1[i], [tau]_2)   == e(sum_i rho_i g1[i+1], [1]_2)     i = 0 .. 4094: the two sums are the verifier's bucket MSMs
//   e(g1[0], sum_j rho'_j g2[j+1]) == e(g1[1], sum_j rho'_j g2[j])       j = 0 .. 63: 64-term sums on the host
// (a chain that is not geometric passes with probability 2^-128).  That g1[0] and g2[0] are the standard generators was checked
// on the bytes (trusted_setup.cpp).  Throws with a message that says which chain failed.
void Engine::check_setup_powers() {
    const TrustedSetup& ts = *setup_;
    {
        std::vector<uint32_t> w((size_t)(N_BLOB - 1) * 4);
        ts.weights128(1, reinterpret_cast<uint32_t(*)[4]>(w.data()), N_BLOB - 1);
        std::vector<Fr8> s0((size_t)N_BLOB - 1), s1((size_t)N_BLOB);  // canonical scalars: the weights are below 2^128 < r
        memset(s0.data(), 0, s0.size() * sizeof(Fr8));
        memset(s1.data(), 0, s1.size() * sizeof(Fr8));
        for (int i = 0; i < N_BLOB - 1; i++) {
            memcpy(s0[(size_t)i].v, &w[(size_t)i * 4], 16);      // job 0: sum rho_i g1[i], pairs with [tau]_2
            memcpy(s1[(size_t)i + 1].v, &w[(size_t)i * 4], 16);  // job 1: sum rho_i g1[i+1], pairs with -[1]_2
        }
        if (!pairing_check_4844(d_srs_, s0, s1)) throw std::runtime_error("g1_monomial is not a sequence of consecutive powers of the tau of g2_monomial[1] (wrong basis or order?)");
    }
    {
        constexpr int M = (int)TrustedSetup::N_G2 - 1;
        std::vector<pairing::G2Affine> q(TrustedSetup::N_G2);
        for (size_t j = 0; j < TrustedSetup::N_G2; j++)
            if (!pairing::g2_decompress(q[j], ts.g2.data() + j * TrustedSetup::G2_BYTES)) throw std::runtime_error("trusted setup: G2 point failed to decompress");
        uint32_t w[M][4];
        ts.weights128(2, w, M);
        const pairing::G2Prepared hi = pairing::prepare(pairing::g2_lincomb128(q.data() + 1, w, M));
        const pairing::G2Prepared lo = pairing::prepare(pairing::g2_neg(pairing::g2_lincomb128(q.data(), w, M)));
        G1Affine P[2];
        HIPCK(hipMemcpy(P, d_srs_, sizeof P, hipMemcpyDeviceToHost));
        const pairing::G2Prepared* qq[2] = {&hi, &lo};
        if (!pairing::product_is_one(P, qq, 2)) throw std::runtime_error("g2_monomial is not a sequence of consecutive powers of the tau of g1_monomial[1]");
    }
}

static Fr8 canon8(const Fr& mont) { return to8(from_mont(mont)); }

// Verifier::verify_kzg_proof (kzg_single_open/src/verifier.rs:33-57): e(C - yG, -G2) e(pi, [tau - z]_2) == 1, evaluated as
// e(C - yG + z pi, -G2) e(pi, [tau]_2) == 1 (bilinearity; the shape the reference's batch verifier uses, :76-107).
int Engine::verify_kzg_proof_host(const uint8_t* commitment, const uint8_t* z_bytes, const uint8_t* y_bytes, const uint8_t* proof,
                                  int* verified) {
    *verified = 0;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        // point array [pi | C | G]
        PoolBuf d_pts(*this, 3 * sizeof(G1Affine));
        uint8_t two[96];
        memcpy(two, proof, 48);
        memcpy(two + 48, commitment, 48);
        int pst[2];
        check_points(this, two, 2, d_pts.p, pst, stream_, beta_);
        if (pst[1]) return ERR_G1;  // commitment first, then proof (eip4844/src/verifier.rs:29-33)
        if (pst[0]) return ERR_G1;
        Fr z, y;
        if (!fr_from_be_canonical(z, z_bytes)) return ERR_SCALAR;
        if (!fr_from_be_canonical(y, y_bytes)) return ERR_SCALAR;
        launch::copy_affine(d_srs_, (G1Affine*)d_pts.p + 2, 1, stream_);  // G = [1]_1 = g1_monomial[0]
        std::vector<Fr8> s0 = {canon8(one<FrParams>())};
        std::vector<Fr8> s1 = {canon8(z), canon8(one<FrParams>()), canon8(neg(y))};
        *verified = pairing_check_4844(d_pts.p, s0, s1);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// The second half of verify_blob_kzg_proof_batch, shared by the host and the device-resident form: the challenges z_i (Montgomery)
// and evaluations y_i (canonical) are known, d_points = [proofs n | commitments n | room for G] holds the decoded points.
// Hashes the weight r on the host (one short message), forms the two scalar lists and runs the bucket MSMs + pairing.  Returns 1 / 0.
int Engine::finish_verify_blob_batch(int n, const Fr8* z_mont, const Fr8* y_canon, const uint8_t* const* commitments,
                                     const uint8_t* const* proofs, const void* d_points, G1Affine* sums2) {
    void* d_pts = const_cast<void*>(d_points);
    launch::copy_affine(d_srs_, (G1Affine*)d_pts + 2 * n, 1, stream_);
    std::vector<Fr> zs(n), ys(n);
    for (int i = 0; i < n; i++) { zs[i] = from8(z_mont[i]); ys[i] = from8(y_canon[i]); }
    const Fr r = blob_batch_weight(n, commitments, zs.data(), ys.data(), proofs);
    // lhs = sum r^i C_i - (sum r^i y_i) G + sum r^i z_i pi_i ; rhs = sum r^i pi_i   (kzg_single_open/src/verifier.rs:76-99)
    std::vector<Fr8> s0(n), s1(2 * n + 1);
    Fr cur = one<FrParams>(), ysum = zero<FrParams>();
    for (int i = 0; i < n; i++) {
        s0[i] = canon8(cur);
        s1[i] = canon8(mul(cur, zs[i]));
        s1[n + i] = s0[i];
        ysum = add(ysum, mul(cur, to_mont(ys[i])));
        cur = mul(cur, r);
    }
    s1[2 * n] = canon8(neg(ysum));
    return pairing_check_4844(d_pts, s0, s1, sums2);
}

int Engine::verify_blob_kzg_proof_batch_host(uint64_t n_blobs, const uint8_t* const* blobs, uint64_t n_commitments,
                                             const uint8_t* const* commitments, uint64_t n_proofs, const uint8_t* const* proofs,
                                             int* verified, G1Affine* sums2) {
    *verified = 0;
    if (!(n_blobs == n_commitments && n_blobs == n_proofs)) return ERR_INPUT;  // eip4844/src/verifier.rs:87-95
    const int n = (int)n_blobs;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        // challenges z_i and evaluations y_i = p_i(z_i)
        std::vector<Fr8> z8(n), y8(n);
        std::vector<int> bst(n);
        for (int i = 0; i < n; i++) z8[i] = to8(blob_challenge(blobs[i], commitments[i]));
        if (n) open_blobs_at(n, blobs, z8.data(), false, nullptr, y8.data(), bst.data());
        for (int i = 0; i < n; i++) if (bst[i]) return ERR_SCALAR;          // blobs first,
        // point array [proofs n | commitments n | G]
        PoolBuf d_pts(*this, (size_t)(2 * n + 1) * sizeof(G1Affine));
        std::vector<uint8_t> pb((size_t)2 * n * 48 + 1);
        std::vector<int> pst(2 * n + 1);
        for (int i = 0; i < n; i++) { memcpy(&pb[(size_t)i * 48], proofs[i], 48); memcpy(&pb[(size_t)(n + i) * 48], commitments[i], 48); }
        if (n) check_points(this, pb.data(), 2 * n, d_pts.p, pst.data(), stream_, beta_);
        for (int i = 0; i < n; i++) if (pst[n + i]) return ERR_G1;          // then commitments,
        for (int i = 0; i < n; i++) if (pst[i]) return ERR_G1;              // then proofs (verifier.rs:97-113)
        *verified = finish_verify_blob_batch(n, z8.data(), y8.data(), commitments, proofs, d_pts.p, sums2);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// verify_blob_kzg_proof (eip4844/src/verifier.rs:50-76): single-opening check at the Fiat-Shamir point
int Engine::verify_blob_kzg_proof_host(const uint8_t* blob, const uint8_t* commitment, const uint8_t* proof, int* verified) {
    *verified = 0;
    std::lock_guard<std::recursive_mutex> whole_call(mu_);
    int st = OK;
    Fr z, y;
    {
        std::lock_guard<std::recursive_mutex> lk(mu_);
        try {
            HIPCK(hipSetDevice(dev_));
            z = blob_challenge(blob, commitment);
            Fr8 z8 = to8(z), y8;
            int bst = 0;
            const uint8_t* bl[1] = {blob};
            open_blobs_at(1, bl, &z8, false, nullptr, &y8, &bst);
            if (bst) return ERR_SCALAR;
            y = from8(y8);
        } catch (const std::exception& e) {
            set_error(e);
            return ERR_DEVICE;
        }
    }
    uint8_t zb[32], yb[32];
    fr_to_be(zb, from_mont(z));
    fr_to_be(yb, y);
    st = verify_kzg_proof_host(commitment, zb, yb, proof, verified);
    return st;
}

// ---------------------------------------------------------------------------------------------
// Batched and device-resident forms (include/c_eth_kzg.h: eth_kzg_amd_compute_*_kzg_proof_batch / _device,
// eth_kzg_amd_verify_blob_kzg_proof_batch_device).  One opening core per (sub-)batch instead of one per blob.

// the engine-owned scratch of these forms, carved from one allocation: [32-byte Fiat-Shamir header | per blob: digest, z, y,
// decoded commitment, proof, four status words].  Grown under mu_; a call that may still use the old block on another stream
// has recorded work_[0].done, and hipFree waits for the device.
Engine::Scratch4844 Engine::scratch_4844(int n) {
    constexpr size_t HDR = 256;  // keeps every array 16-byte aligned
    if (n > cap_4844_) {
        const int cap = ((n + 63) / 64) * 64;
        if (d_4844_) { HIPCK(hipFree(d_4844_)); d_4844_ = nullptr; cap_4844_ = 0; }
        HIPCK(hipMalloc(&d_4844_, HDR + (size_t)cap * (32 + 32 + 32 + sizeof(G1Affine) + 48 + 4 * sizeof(int))));
        uint8_t hdr[32];  // compute_fiat_shamir_challenge's domain separator and degree, as the host's blob_challenge hashes them
        blob_challenge_header(hdr);
        HIPCK(hipMemcpy(d_4844_, hdr, 32, hipMemcpyHostToDevice));
        cap_4844_ = cap;
    }
    const size_t cap = (size_t)cap_4844_;
    uint8_t* p = (uint8_t*)d_4844_ + HDR;
    Scratch4844 s;
    s.dig = p; p += cap * 32;
    s.z = p; p += cap * 32;
    s.y = p; p += cap * 32;
    s.aff = p; p += cap * sizeof(G1Affine);
    s.proofs = p; p += cap * 48;
    s.blob_bad = (int*)p; p += cap * sizeof(int);
    s.z_bad = (int*)p; p += cap * sizeof(int);
    s.g1_bad = (int*)p; p += cap * sizeof(int);
    s.status = (int*)p;
    return s;
}
// z_i = H(blob_challenge_header | blob_i | commitment_i) mod r for blobs and commitments in HBM: one lane per blob hashes
// (k_sha256.hip), one lane per digest reduces (k_4844.hip); s.z then feeds k_quotient_by_linear without a host round trip
void Engine::fs_challenges_device(int n, const uint8_t* d_blobs, const uint8_t* d_commitments, const Scratch4844& s, hipStream_t st) {
    launch::sha256_many(n, (const uint8_t*)d_4844_, 32, d_blobs, BYTES_PER_BLOB, BYTES_PER_BLOB, d_commitments, 48, 48, s.dig, st);
    launch::fr_from_be32(n, s.dig, s.z, nullptr, /*reduce=*/true, st);
}

int Engine::compute_blob_kzg_proof_device(int n, const uint8_t* d_blobs, const uint8_t* d_commitments, uint8_t* d_out_proofs, int* h_status,
                                          hipStream_t st, bool sync) {
    if (n <= 0) return OK;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    if (n > device_batch_max_) {  // sub-batches (0.5 MB of scratch per blob), as blob_to_kzg_commitment_device
        for (int b0 = 0; b0 < n; b0 += device_batch_max_) {
            const int nb = std::min(device_batch_max_, n - b0);
            const int rc = compute_blob_kzg_proof_device(nb, d_blobs + (size_t)b0 * BYTES_PER_BLOB, d_commitments + (size_t)b0 * 48,
                                                         d_out_proofs + (size_t)b0 * 48, h_status ? h_status + b0 : nullptr, st, sync);
            if (rc) return rc;
        }
        return OK;
    }
    try {
        HIPCK(hipSetDevice(dev_));
        if (!st) {  // NULL: the library's stream, ordered behind whatever the caller has queued on the default stream so far
            st = stream_;
            HIPCK(hipEventRecord(work_[0].ev_in, nullptr));
            HIPCK(hipStreamWaitEvent(st, work_[0].ev_in, 0));
        }
        ensure_workspace(n);
        const Scratch4844 s = scratch_4844(n);
        HIPCK(hipStreamWaitEvent(st, work_[0].done, 0));  // an earlier asynchronous call on another stream may still use the workspace
        fs_challenges_device(n, d_blobs, d_commitments, s, st);
        open_blobs_core(n, d_blobs, s.z, s.y, d_out_proofs, st);
        if (h_status) {  // the commitment is only validated (prover.rs:73-75): without a status array there is nobody to tell
            launch::g1_decompress(d_commitments, s.aff, s.g1_bad, n, 1, beta_, st);
            launch::status_4844(n, d_status_, nullptr, s.g1_bad, s.status, st);
            HIPCK(hipMemcpyAsync(h_status, s.status, n * sizeof(int), hipMemcpyDeviceToHost, st));
        }
        HIPCK(hipEventRecord(work_[0].done, st));
        HIPCK(hipGetLastError());
        if (sync || h_status) HIPCK(hipStreamSynchronize(st));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

int Engine::compute_kzg_proof_device(int n, const uint8_t* d_blobs, const uint8_t* d_z, uint8_t* d_out_proofs, uint8_t* d_out_y, int* h_status,
                                     hipStream_t st, bool sync) {
    if (n <= 0) return OK;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    if (n > device_batch_max_) {
        for (int b0 = 0; b0 < n; b0 += device_batch_max_) {
            const int nb = std::min(device_batch_max_, n - b0);
            const int rc = compute_kzg_proof_device(nb, d_blobs + (size_t)b0 * BYTES_PER_BLOB, d_z + (size_t)b0 * 32, d_out_proofs + (size_t)b0 * 48,
                                                    d_out_y + (size_t)b0 * 32, h_status ? h_status + b0 : nullptr, st, sync);
            if (rc) return rc;
        }
        return OK;
    }
    try {
        HIPCK(hipSetDevice(dev_));
        if (!st) {
            st = stream_;
            HIPCK(hipEventRecord(work_[0].ev_in, nullptr));
            HIPCK(hipStreamWaitEvent(st, work_[0].ev_in, 0));
        }
        ensure_workspace(n);
        const Scratch4844 s = scratch_4844(n);
        HIPCK(hipStreamWaitEvent(st, work_[0].done, 0));
        launch::fr_from_be32(n, d_z, s.z, s.z_bad, /*reduce=*/false, st);  // canonicity is checked on the device; a bad z opens at 0
        open_blobs_core(n, d_blobs, s.z, s.y, d_out_proofs, st);
        launch::fr_to_be32(n, s.y, d_out_y, st);
        if (h_status) {
            launch::status_4844(n, d_status_, s.z_bad, nullptr, s.status, st);  // the blob's own check first, then z: the single call's order
            HIPCK(hipMemcpyAsync(h_status, s.status, n * sizeof(int), hipMemcpyDeviceToHost, st));
        }
        HIPCK(hipEventRecord(work_[0].done, st));
        HIPCK(hipGetLastError());
        if (sync || h_status) HIPCK(hipStreamSynchronize(st));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// The two host-pointer forms.  Per sub-batch of 256 blobs: the helper threads gather the blobs into pinned memory and, the bytes
// being in their cache anyway, hash the challenge (a SHA-NI core is faster per message than a GPU lane) or parse z; one upload, one
// core, one download.  commitments != null: compute_blob_kzg_proof; zs != null: compute_kzg_proof.
int Engine::proofs_batch_host(int n, const uint8_t* const* blobs, const uint8_t* const* commitments, const uint8_t* const* zs,
                              uint8_t* const* out_proofs, uint8_t* const* out_ys, int* h_status) {
    constexpr int SUB = 256;
    HostPool* pool = n >= 4 ? ensure_host_pool() : nullptr;  // a couple of blobs: everything on the calling thread
    for (int b0 = 0; b0 < n; b0 += SUB) {
        const int nb = std::min(SUB, n - b0);
        PoolBuf h_in(*this, (size_t)nb * BYTES_PER_BLOB, /*pinned_host=*/true);
        std::vector<Fr8> z8(nb);
        std::vector<int> z_ok(nb, 1), bst(nb), cst(nb, 0);
        std::vector<uint8_t> cm(commitments ? (size_t)nb * 48 : 0), pr((size_t)nb * 48);
        std::vector<Fr8> y8(nb);
        parallel_for(nb, pool ? pool->threads() + 1 : 1, pool, [&](int i) {
            uint8_t* dst = (uint8_t*)h_in.p + (size_t)i * BYTES_PER_BLOB;
            memcpy(dst, blobs[b0 + i], BYTES_PER_BLOB);
            Fr z;
            if (commitments) {
                memcpy(&cm[(size_t)i * 48], commitments[b0 + i], 48);
                z = blob_challenge(dst, &cm[(size_t)i * 48]);
            } else if (!fr_from_be_canonical(z, zs[b0 + i])) {
                z_ok[i] = 0;
                z = zero<FrParams>();
            }
            z8[i] = to8(z);
        });
        open_staged_blobs(nb, (const uint8_t*)h_in.p, z8.data(), commitments ? cm.data() : nullptr, pr.data(), y8.data(), bst.data(), cst.data());
        for (int i = 0; i < nb; i++) {
            const int st = bst[i] ? ERR_SCALAR : !z_ok[i] ? ERR_SCALAR : cst[i] ? ERR_G1 : OK;  // the single call's order
            if (h_status) h_status[b0 + i] = st;
            if (st) continue;
            memcpy(out_proofs[b0 + i], &pr[(size_t)i * 48], 48);
            if (out_ys) fr_to_be(out_ys[b0 + i], from8(y8[i]));
        }
    }
    return OK;
}

// one sub-batch of the host forms on stream_: pinned blobs up, core, (commitments validated,) results down
void Engine::open_staged_blobs(int nb, const uint8_t* h_blobs_pinned, const Fr8* z_mont, const uint8_t* h_commitments, uint8_t* h_proofs,
                               Fr8* h_y, int* h_blob_status, int* h_g1_status) {
    hipStream_t st = stream_;
    ensure_workspace(nb);
    PoolBuf d_in(*this, (size_t)nb * BYTES_PER_BLOB), d_z(*this, (size_t)nb * 32), d_y(*this, (size_t)nb * 32), d_pr(*this, (size_t)nb * 48);
    PoolBuf d_cm(*this, (size_t)nb * 48), d_aff(*this, (size_t)nb * sizeof(G1Affine)), d_cst(*this, (size_t)nb * sizeof(int));
    HIPCK(hipMemcpyAsync(d_in.p, h_blobs_pinned, (size_t)nb * BYTES_PER_BLOB, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(d_z.p, z_mont, (size_t)nb * 32, hipMemcpyHostToDevice, st));
    open_blobs_core(nb, (const uint8_t*)d_in.p, d_z.p, d_y.p, (uint8_t*)d_pr.p, st);
    if (h_commitments) {
        HIPCK(hipMemcpyAsync(d_cm.p, h_commitments, (size_t)nb * 48, hipMemcpyHostToDevice, st));
        launch::g1_decompress((const uint8_t*)d_cm.p, d_aff.p, (int*)d_cst.p, nb, 1, beta_, st);  // only validated (prover.rs:73-75)
        HIPCK(hipMemcpyAsync(h_g1_status, d_cst.p, nb * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    HIPCK(hipMemcpyAsync(h_proofs, d_pr.p, (size_t)nb * 48, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(h_y, d_y.p, (size_t)nb * 32, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(h_blob_status, d_status_, nb * sizeof(int), hipMemcpyDeviceToHost, st));
    SYNC_CHECKED(st);
}

int Engine::compute_blob_kzg_proof_batch_host(int n, const uint8_t* const* blobs, const uint8_t* const* commitments, uint8_t* const* out_proofs,
                                              int* h_status) {
    if (n <= 0) return OK;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        proofs_batch_host(n, blobs, commitments, nullptr, out_proofs, nullptr, h_status);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}
int Engine::compute_kzg_proof_batch_host(int n, const uint8_t* const* blobs, const uint8_t* const* zs, uint8_t* const* out_proofs,
                                         uint8_t* const* out_ys, int* h_status) {
    if (n <= 0) return OK;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        proofs_batch_host(n, blobs, nullptr, zs, out_proofs, out_ys, h_status);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// verify_blob_kzg_proof_batch on flat arrays in HBM.  GPU: challenges (hash + reduction), y_i = p_i(z_i) through the core in
// sub-batches, commitments and proofs decompressed where they lie.  Down: z, y, the status words and the 96 n point bytes the
// weights' transcript hashes.  Then exactly the host form's second half.
int Engine::verify_blob_kzg_proof_batch_device(uint64_t n64, const uint8_t* d_blobs, const uint8_t* d_commitments, const uint8_t* d_proofs,
                                               int* verified, hipStream_t user_stream, G1Affine* sums2) {
    *verified = 0;
    if (n64 == 0) { *verified = 1; return OK; }  // an empty batch verifies, as in the host form
    if (n64 > (1u << 24)) return ERR_INPUT;
    const int n = (int)n64;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        std::vector<Fr8> z8(n), y8(n);  // inside the try: allocations must not unwind through the C ABI
        std::vector<int> bst(n), pst(2 * (size_t)n);
        std::vector<uint8_t> pb((size_t)2 * n * 48);
        std::vector<const uint8_t*> cp(n), pp(n);
        HIPCK(hipSetDevice(dev_));
        hipStream_t st = stream_;
        order_behind(st, user_stream, v_decoded_);
        const int sub = std::min(n, device_batch_max_);
        ensure_workspace(sub);
        const Scratch4844 s = scratch_4844(n);
        fs_challenges_device(n, d_blobs, d_commitments, s, st);
        for (int b0 = 0; b0 < n; b0 += sub) {
            const int nb = std::min(sub, n - b0);
            open_blobs_core(nb, d_blobs + (size_t)b0 * BYTES_PER_BLOB, (const uint8_t*)s.z + (size_t)b0 * 32, (uint8_t*)s.y + (size_t)b0 * 32, nullptr, st);
            HIPCK(hipMemcpyAsync(s.blob_bad + b0, d_status_, nb * sizeof(int), hipMemcpyDeviceToDevice, st));
        }
        // point array [proofs n | commitments n | G], decoded and subgroup-checked from where the bytes lie
        PoolBuf d_pts(*this, (size_t)(2 * n + 1) * sizeof(G1Affine)), d_pst(*this, (size_t)2 * n * sizeof(int));
        launch::g1_decompress2(d_proofs, d_pts.p, (int*)d_pst.p, n, d_commitments, (G1Affine*)d_pts.p + n, (int*)d_pst.p + n, n, beta_, st);
        HIPCK(hipMemcpyAsync(z8.data(), s.z, (size_t)n * 32, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(y8.data(), s.y, (size_t)n * 32, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(bst.data(), s.blob_bad, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(pst.data(), d_pst.p, (size_t)2 * n * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(pb.data(), d_proofs, (size_t)n * 48, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(pb.data() + (size_t)n * 48, d_commitments, (size_t)n * 48, hipMemcpyDeviceToHost, st));
        SYNC_CHECKED(st);
        for (int i = 0; i < n; i++) if (bst[i]) return ERR_SCALAR;          // blobs first,
        for (int i = 0; i < n; i++) if (pst[n + i]) return ERR_G1;          // then commitments,
        for (int i = 0; i < n; i++) if (pst[i]) return ERR_G1;              // then proofs (verifier.rs:97-113)
        for (int i = 0; i < n; i++) { pp[i] = pb.data() + (size_t)i * 48; cp[i] = pb.data() + (size_t)(n + i) * 48; }
        *verified = finish_verify_blob_batch(n, z8.data(), y8.data(), cp.data(), pp.data(), d_pts.p, sums2);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

}  // namespace kzg
