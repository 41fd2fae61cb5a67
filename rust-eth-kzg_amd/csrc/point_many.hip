// eth_kzg_amd_verify_kzg_proof_many / _many_device: MANY independent verify_kzg_proof items (commitment, z, y, proof) in one call, a
// verdict and a status for each -- per item exactly what Verifier::verify_kzg_proof says of it alone (crates/eip4844/src/verifier.rs:
// 19-44; eip4844.hip: verify_kzg_proof_host is the single call and is not touched).  The statement of the check -- leaves, seed, weights,
// the pair of a range, why a passing full-range pair means valid items only -- is verify_host.hpp (PointProofTranscript).
// A call is cut into passes of at most POINT_MANY_PASS items; a pass runs on a PASS SLOT of the many-verification (verify_many.hip: the
// slot's own lock, arena, pinned slab and stream; nothing here takes the context's big lock), and a call of several passes runs them on
// up to three slots side by side: one pass's staging, hashing and pairings on the host threads under another's products on the GPU.
//   host threads : host form: gather the items into the pinned slab, one SHA-256 leaf per item (behind the GPU's decoding); both forms:
//                  the seed and the weights, ONE 2-pairing check of the full-range pair per pass, and only if that fails the SEARCH of
//                  vm_search.hpp over sub-ranges of the resident pairs, down to single items (single items are probes like the others:
//                  the per-item pairs never come down)
//   GPU          : device form: the four arrays device-to-device into the arena (from any byte address), the leaves' bodies gathered
//                  and hashed (k_pm_leaf_bodies, k_sha256_many); both: g1_decompress2 of [proofs | commitments], fr_from_be32 of z and
//                  y, the status words, then the four scalar multiplications per item, one lane each (k_point_many.hip: k_pm_mul), the
//                  per-item pairs (k_pm_pairs), and the full-range fold in TWO LEVELS of k_vm_fold_ranges: ranges of 128 items, one
//                  block each, then one block over those sums.  (k_vm_fold_sum's single block would add 128 points per lane one
//                  after the other at 16384 items, a serial tail of ~130 dependent additions behind products that fill the chip; the
//                  two levels are 1 + 7 and 1 + 7 dependent additions.)
// Down the link go the status words, the n x 32 leaf digests (device form) and the sums; up go the weights (and the host form's items).
// THE BLOB SOURCE (eth_kzg_amd_verify_blob_kzg_proof_many / _many_device; the statement: verify_host.hpp): the item comes as (blob,
// commitment, proof) and the pass makes z and y itself, then is the pass above from "decoding" on.
//   host threads : host form: gather the blobs (128 KB each) into the pinned slab and, the bytes being in their cache, hash blob_challenge
//                  (eip4844.hip: proofs_batch_host says why the host hashes what it holds); ONE upload of blobs, proofs, commitments, z
//   GPU          : device form: proofs and commitments device-to-device into the arena, z = k_sha256_many over the caller's blobs WHERE
//                  THEY LIE plus the arena's commitments, behind a header the slot owns, reduced by fr_from_be32; both: y = p(z) by
//                  k_blob_eval_at (k_ntt.hip: inside the CU, no workspace), the leaves' bodies gathered and hashed on the GPU -- y exists
//                  only there --, the merged status (k_pm_blob_status), then the products as above
// Nothing of it takes mu_, calls ensure_workspace or touches the engine's coefficient arrays: d_w29_ and n_inv4096_ are constants.
#include "vm_search.hpp"

namespace kzg {

namespace {
constexpr int FOLD_SPAN = 128;  // items per first-level range of the full-range fold: one per lane of k_vm_fold_ranges' trees

struct PointPassLayout {
    const int n;
    const int blobs;  // 0: the items bring z and y; 1: blobs staged through the slab (host form); 2: blobs read where they lie (device form)
    const int n_l1 = (n + FOLD_SPAN - 1) / FOLD_SPAN;  // first-level ranges of the full-range fold
    // probes per batch of the search: a pass's worth, so that "every live suspect on its own" is ONE launch of k_pairing_check (a wave of
    // it takes as long as a thousand; 5.5 MB of range sums on either side at 16384)
    const int max_ranges = n;
    static constexpr size_t JACQ = launch::SIZEOF_JACQ;
    Carve d;  // (members are initialised in the order they stand here)
    // the blob source's own arrays take no room otherwise (Carve: an array of no bytes): the other sources' layout is what it was
    const size_t off_blob = d.take(blobs == 1 ? (size_t)n * BYTES_PER_BLOB : 0), off_hdr = d.take(blobs == 2 ? 32 : 0);
    // inputs: one upload in the host form, device-to-device copies in the device form; then the fold's ranges and the weights
    const size_t off_p = d.take((size_t)n * 48), off_c = d.take((size_t)n * 48), off_z = d.take((size_t)n * 32), off_y = d.take((size_t)n * 32),
                 in_bytes = d.end, off_frng = d.take((size_t)(n_l1 + 1) * 8), off_rho = d.take((size_t)n * 16), in2_bytes = d.end;
    Carve h = d;  // pinned read-backs behind the inputs
    const size_t poff_st = h.take((size_t)n * 4), poff_fold = h.take(2 * JACQ), poff_rng = h.take((size_t)max_ranges * 8),
                 poff_rsum = h.take((size_t)2 * max_ranges * JACQ), poff_leaf = h.take((size_t)n * 32), poff_verd = h.take((size_t)max_ranges), pin_bytes = h.end;
    // device only
    const size_t off_pts = d.take((size_t)2 * n * sizeof(G1Affine)), off_stp = d.take((size_t)2 * n * 4), off_zbad = d.take((size_t)n * 4),
                 off_ybad = d.take((size_t)n * 4), off_st = d.take((size_t)n * 4), off_zm = d.take((size_t)n * sizeof(Fr)),
                 off_ym = d.take((size_t)n * sizeof(Fr)), off_pairs = d.take((size_t)2 * n * JACQ), off_terms = d.take((size_t)3 * n * JACQ),
                 off_l1 = d.take((size_t)2 * n_l1 * JACQ), off_fold = d.take(2 * JACQ), off_rng = d.take((size_t)max_ranges * 8),
                 off_rsum = d.take((size_t)2 * max_ranges * JACQ), off_bodies = d.take((size_t)n * PointProofTranscript::LEAF_BYTES),
                 off_leaf = d.take((size_t)n * 32), off_dig = d.take(blobs == 2 ? (size_t)n * 32 : 0), off_bbad = d.take(blobs ? (size_t)n * 4 : 0),
                 off_verd = d.take((size_t)max_ranges),  // the verdict bytes of k_pairing_check
                 dev_bytes = d.end;
    explicit PointPassLayout(int n_, int blobs_) : n(n_), blobs(blobs_) {}
};
}  // namespace

// One pass: items [lo, lo + n) of the call on a pass slot, its steps in the order run() takes them.  Everything goes onto the slot's
// stream st; the tap (null in the product) is the call's.
struct Engine::PointPass {
    Engine& e;
    const PointManyInput src;  // the call's input from lo on
    const uint64_t lo;
    const int n, pass;
    int *const ver, *const stat;  // the pass's verdicts and statuses in the caller's arrays
    PointManyTap* const tap;
    const int T;
    HostPool* const pool;
    PassSlot slot = e.lease_pass_slot(/*prefer_idle_work_set=*/true);
    const hipStream_t st = slot.stream;
    TraceLap lap{e.knobs_.trace, src.from_blobs ? "verify_blob_kzg_proof_many" : "verify_kzg_proof_many"};
    const PointPassLayout L{n, !src.from_blobs ? 0 : src.on_device ? 2 : 1};
    const pairing::G2Prepared* const vk[2] = {e.g2_tau1_.get(), e.g2_neg_gen_.get()};  // [tau]_2, -[1]_2: the single call's (eip4844.hip)
    uint8_t *hb = nullptr, *db = nullptr;  // the slot's pinned slab and device arena
    std::vector<char> live;                // items that decoded without an error
    int n_live = 0;
    int* h_st() const { return (int*)(hb + L.poff_st); }
    uint8_t* h_leaf() const { return hb + L.poff_leaf; }

    void run() {
        arena();
        stage_items();
        decode_and_status();
        weights_and_ranges();
        products_and_fold();
        verdicts();
    }
    // the slot's blocks, large enough; stale contents of the persistent slab must fail closed: status words and result slots are poisoned
    void arena() {
        HIPCK(hipSetDevice(e.dev_));
        grow_device(slot.slot->dev, slot.slot->dev_cap, L.dev_bytes, st);
        grow_pinned(slot.slot->pin, slot.slot->pin_cap, L.pin_bytes);
        hb = slot.slot->pin;
        db = (uint8_t*)slot.slot->dev;
        memset(h_st(), 0xff, (size_t)n * 4);
        memset(hb + L.poff_fold, 0xff, 2 * launch::SIZEOF_JACQ);
        memset(h_leaf(), 0xff, (size_t)n * 32);
        HIPCK(hipMemsetAsync(db + L.off_st, 0xff, (size_t)n * 4, st));
        HIPCK(hipMemsetAsync(db + L.off_stp, 0xff, (size_t)2 * n * 4, st));
        HIPCK(hipMemsetAsync(db + L.off_fold, 0xff, 2 * launch::SIZEOF_JACQ, st));
    }
    // the leaves of items whose z and y are in the arena: bodies gathered and hashed on the GPU, the digests down
    void leaves_on_gpu() {
        launch::pm_leaf_bodies(db + L.off_c, db + L.off_z, db + L.off_y, db + L.off_p, db + L.off_bodies, n, st);
        launch::sha256_many(n, nullptr, 0, db + L.off_bodies, PointProofTranscript::LEAF_BYTES, (uint32_t)PointProofTranscript::LEAF_BYTES, nullptr, 0, 0,
                            db + L.off_leaf, st);
        HIPCK(hipMemcpyAsync(h_leaf(), db + L.off_leaf, (size_t)n * 32, hipMemcpyDeviceToHost, st));
    }
    // ---- the items into the arena, from one of the three sources
    void stage_items() {
        if (src.on_device) order_behind(st, src.user_stream, slot.slot->ordered);
        if (src.from_blobs) {
            const uint8_t* d_blobs = nullptr;
            if (src.on_device) {
                blob_challenge_header(hb + L.off_hdr);  // the slot's own copy of the 32 bytes (the engine's lives under mu_)
                HIPCK(hipMemcpyAsync(db + L.off_hdr, hb + L.off_hdr, 32, hipMemcpyHostToDevice, st));
                HIPCK(hipMemcpyAsync(db + L.off_p, src.d_proofs, (size_t)n * 48, hipMemcpyDeviceToDevice, st));
                HIPCK(hipMemcpyAsync(db + L.off_c, src.d_commitments, (size_t)n * 48, hipMemcpyDeviceToDevice, st));
                d_blobs = src.d_blobs;
                launch::sha256_many(n, db + L.off_hdr, 32, d_blobs, BYTES_PER_BLOB, BYTES_PER_BLOB, db + L.off_c, 48, 48, db + L.off_dig, st);
                launch::fr_from_be32(n, db + L.off_dig, db + L.off_zm, nullptr, /*reduce=*/true, st);
                launch::fr_mont_to_be32(n, db + L.off_zm, db + L.off_z, st);
            } else {
                parallel_for(n, T, pool, [&](int i) {
                    uint8_t* const blob = hb + L.off_blob + (size_t)i * BYTES_PER_BLOB;
                    memcpy(blob, src.blobs[i], BYTES_PER_BLOB);
                    memcpy(hb + L.off_p + (size_t)i * 48, src.proofs[i], 48);
                    memcpy(hb + L.off_c + (size_t)i * 48, src.commitments[i], 48);
                    fr_to_be(hb + L.off_z + (size_t)i * 32, from_mont(blob_challenge(blob, hb + L.off_c + (size_t)i * 48)));
                });
                lap("stage + challenges (host)");
                HIPCK(hipMemcpyAsync(db, hb, L.off_y, hipMemcpyHostToDevice, st));  // blobs | proofs | commitments | z
                d_blobs = db + L.off_blob;
                launch::fr_from_be32(n, db + L.off_z, db + L.off_zm, (int*)(db + L.off_zbad), /*reduce=*/false, st);  // (a reduced digest: never refused)
            }
            launch::blob_eval_at(n, d_blobs, db + L.off_zm, db + L.off_y, db + L.off_ym, (int*)(db + L.off_bbad), e.d_w29_, e.n_inv4096_, st);
            leaves_on_gpu();  // (y exists only there)
            if (tap) {  // the pinned staging rows of z and y are free behind the upload
                HIPCK(hipMemcpyAsync(hb + L.off_z, db + L.off_z, (size_t)n * 32, hipMemcpyDeviceToHost, st));
                HIPCK(hipMemcpyAsync(hb + L.off_y, db + L.off_y, (size_t)n * 32, hipMemcpyDeviceToHost, st));
            }
        } else if (src.on_device) {
            HIPCK(hipMemcpyAsync(db + L.off_p, src.d_proofs, (size_t)n * 48, hipMemcpyDeviceToDevice, st));
            HIPCK(hipMemcpyAsync(db + L.off_c, src.d_commitments, (size_t)n * 48, hipMemcpyDeviceToDevice, st));
            HIPCK(hipMemcpyAsync(db + L.off_z, src.d_zs, (size_t)n * 32, hipMemcpyDeviceToDevice, st));
            HIPCK(hipMemcpyAsync(db + L.off_y, src.d_ys, (size_t)n * 32, hipMemcpyDeviceToDevice, st));
            leaves_on_gpu();
        } else {
            parallel_for(n, T, pool, [&](int i) {
                memcpy(hb + L.off_p + (size_t)i * 48, src.proofs[i], 48);
                memcpy(hb + L.off_c + (size_t)i * 48, src.commitments[i], 48);
                memcpy(hb + L.off_z + (size_t)i * 32, src.zs[i], 32);
                memcpy(hb + L.off_y + (size_t)i * 32, src.ys[i], 32);
            });
            lap("stage (host)");
            HIPCK(hipMemcpyAsync(db, hb, L.in_bytes, hipMemcpyHostToDevice, st));
        }
    }
    // ---- GPU work that needs no weight: decoding + subgroup tests of [proofs | commitments], z and y, the status words; the host
    // form's leaves meanwhile; then the statuses and the live items
    void decode_and_status() {
        G1Affine* d_pts = (G1Affine*)(db + L.off_pts);
        int* d_stp = (int*)(db + L.off_stp);
        launch::g1_decompress2(db + L.off_p, d_pts, d_stp, n, db + L.off_c, d_pts + n, d_stp + n, n, e.beta_, st);
        if (src.from_blobs) {
            launch::pm_blob_status(d_stp, (const int*)(db + L.off_bbad), (int*)(db + L.off_st), n, st);
        } else {
            launch::fr_from_be32(n, db + L.off_z, db + L.off_zm, (int*)(db + L.off_zbad), /*reduce=*/false, st);
            launch::fr_from_be32(n, db + L.off_y, db + L.off_ym, (int*)(db + L.off_ybad), /*reduce=*/false, st);
            launch::pm_status(d_stp, (const int*)(db + L.off_zbad), (const int*)(db + L.off_ybad), (int*)(db + L.off_st), n, st);
        }
        HIPCK(hipMemcpyAsync(h_st(), db + L.off_st, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipGetLastError());
        lap("enqueue (host)");
        if (!src.on_device && !src.from_blobs) {  // meanwhile, on the host threads: the leaves, from the caller's bytes as they lie in the slab
            parallel_for(n, T, pool, [&](int i) {
                PointProofTranscript::leaf(hb + L.off_c + (size_t)i * 48, hb + L.off_z + (size_t)i * 32, hb + L.off_y + (size_t)i * 32,
                                           hb + L.off_p + (size_t)i * 48, h_leaf() + (size_t)i * 32);
            });
            lap("leaf hashes (host)");
        }
        SYNC_CHECKED(st);
        lap(src.from_blobs ? "challenges + evaluations + decode + leaf hashes (GPU)" : src.on_device ? "decode + leaf hashes (GPU)" : "wait decode");
        live.assign(n, 0);
        for (int i = 0; i < n; i++) {
            const int s = h_st()[i];
            if (s != OK && s != ERR_SCALAR && s != ERR_G1) throw std::runtime_error("point verification pass left no status");
            stat[i] = s;
            if (s == OK) { live[i] = 1; n_live++; }
        }
    }
    // ---- the seed and the weights of ALL the items of the pass; the ranges of the two-level fold
    void weights_and_ranges() {
        uint8_t seed[32];
        PointProofTranscript::seed((uint64_t)n, h_leaf(), seed);
        uint32_t* const h_rho = (uint32_t*)(hb + L.off_rho);
        parallel_for(n, T, pool, [&](int i) { fold_weight(seed, (uint64_t)i, h_rho + 4 * (size_t)i); });
        int* const h_frng = (int*)(hb + L.off_frng);
        for (int r = 0; r < L.n_l1; r++) { h_frng[2 * r] = r * FOLD_SPAN; h_frng[2 * r + 1] = std::min(n, (r + 1) * FOLD_SPAN); }
        h_frng[2 * L.n_l1] = 0; h_frng[2 * L.n_l1 + 1] = L.n_l1;
        lap("seed + weights (host)");
        if (tap) {
            memcpy(tap->leaves.data() + lo * 32, h_leaf(), (size_t)n * 32);
            if (src.from_blobs) {
                memcpy(tap->zs.data() + lo * 32, hb + L.off_z, (size_t)n * 32);
                memcpy(tap->ys.data() + lo * 32, hb + L.off_y, (size_t)n * 32);
            }
            memcpy(tap->seeds.data() + (size_t)pass * 32, seed, 32);
            memcpy(tap->rho.data() + lo * 4, h_rho, (size_t)n * 16);
        }
    }
    // ---- the products, the per-item pairs, the full-range pair (also when no item is live: the pair is then the identity twice)
    void products_and_fold() {
        HIPCK(hipMemcpyAsync(db + L.off_frng, hb + L.off_frng, L.in2_bytes - L.off_frng, hipMemcpyHostToDevice, st));
        launch::pm_mul((G1Affine*)(db + L.off_pts), e.d_srs_, db + L.off_zm, db + L.off_ym, (const uint32_t*)(db + L.off_rho), (const int*)(db + L.off_st),
                       db + L.off_pairs, db + L.off_terms, n, e.beta_, st);
        launch::pm_pairs(db + L.off_terms, db + L.off_pairs, n, st);
        const int* d_frng = (const int*)(db + L.off_frng);
        if (L.n_l1 == 1) {
            launch::vm_fold_ranges(db + L.off_pairs, d_frng, db + L.off_fold, 1, st);
        } else {
            launch::vm_fold_ranges(db + L.off_pairs, d_frng, db + L.off_l1, L.n_l1, st);
            launch::vm_fold_ranges(db + L.off_l1, d_frng + 2 * L.n_l1, db + L.off_fold, 1, st);
        }
        HIPCK(hipMemcpyAsync(hb + L.poff_fold, db + L.off_fold, 2 * launch::SIZEOF_JACQ, hipMemcpyDeviceToHost, st));
        HIPCK(hipGetLastError());
        SYNC_CHECKED(st);
        lap("products + pairs + fold (GPU)");
    }
    // ---- verdicts: ONE pairing check of the full-range pair; only if that fails the search
    void verdicts() {
        const int v = vm::check_pair((const JacQ*)(hb + L.poff_fold), vk);
        if (v < 0) throw std::runtime_error("point verification pass left no folded result");
        if (tap) {
            memcpy(tap->fold.data() + (size_t)pass * 2 * launch::SIZEOF_JACQ, hb + L.poff_fold, 2 * launch::SIZEOF_JACQ);
            tap->fold_verdict[pass] = v;
        }
        if (v == 1) {
            for (int i = 0; i < n; i++) ver[i] = live[i];
        } else {
            std::atomic<int> device_fault{0};
            std::vector<int> probes;
            vm::SearchView S = vm::search_view(L, n, L.off_pairs, T, pool, hb, vk, e.device_pairing(2), live.data(), ver, &device_fault);
            if (tap) { S.tap_probes = &probes; S.tap_probe_sums = &tap->probe_sums; S.tap_device_probes = &tap->device_probes; }
            vm::search_wrong_proofs(S, n_live, db, st);
            if (device_fault.load()) throw std::runtime_error("point verification pass left no result");
            for (size_t q = 0; tap && q + 2 < probes.size(); q += 3) {
                const int rec[4] = {pass, probes[q], probes[q + 1], probes[q + 2]};
                tap->probes.insert(tap->probes.end(), rec, rec + 4);
            }
        }
        lap("pairing checks (host)");
    }
};

int Engine::verify_kzg_proof_many(uint64_t n64, const PointManyInput& in, int* verified, int* status, PointManyTap* tap) {
    const int n_all = (int)n64;
    for (int i = 0; i < n_all; i++) { verified[i] = 0; status[i] = OK; }
    if (n_all == 0) return OK;
    const int P = tap && tap->pass_size > 0 ? tap->pass_size : in.from_blobs ? BLOB_MANY_PASS : POINT_MANY_PASS;
    std::vector<uint64_t> starts;
    for (uint64_t lo = 0; lo < n64; lo = point_pass_end(n64, lo, (uint64_t)P)) starts.push_back(lo);
    starts.push_back(n64);
    const int n_passes = (int)starts.size() - 1;
    if (tap) {
        tap->pass_starts = starts;
        tap->leaves.assign((size_t)n_all * 32, 0);
        if (in.from_blobs) { tap->zs.assign((size_t)n_all * 32, 0); tap->ys.assign((size_t)n_all * 32, 0); }
        tap->rho.assign((size_t)n_all * 4, 0);
        tap->seeds.assign((size_t)n_passes * 32, 0);
        tap->fold.assign((size_t)n_passes * 2 * launch::SIZEOF_JACQ, 0xff);
        tap->fold_verdict.assign(n_passes, -1);
    }
    const VmHost host = vm_host();
    // passes side by side on the pass slots (the tap's arrays are filled in order: a tapped call runs its passes one after the other)
    const int lanes = tap ? 1 : std::min(n_passes, (int)VM_SLOTS);
    const auto thrown = run_side_by_side(lanes, [&](int lane) {
        for (int p = lane; p < n_passes; p += lanes) {
            const uint64_t lo = starts[p];
            PointPass{*this, in.from(lo), lo, (int)(starts[p + 1] - lo), p, verified + lo, status + lo, tap, host.T, host.pool}.run();
        }
    });
    for (int l = 0; l < lanes; l++)
        if (thrown[l]) {
            for (int i = 0; i < n_all; i++) verified[i] = 0;
            set_error(std::runtime_error(what_was_thrown(thrown[l], "", "unknown failure")));
            return ERR_DEVICE;
        }
    return OK;
}

}  // namespace kzg
