// verify_cell_kzg_proof_batch: host orchestration.
// Reference: DASContext::verify_cell_kzg_proof_batch (crates/eip7594/src/verifier.rs:49-164),
// FK20Verifier::{new, verify_multi_opening} (crates/cryptography/kzg_multi_open/src/fk20/verifier.rs:58-260),
// compute_fiat_shamir_challenge (:269-328).
// Work split: all G1 / Fr batch arithmetic on the GPU; the sequential SHA-256 transcript (verify_host.hpp) and the
// constant-size 2-pairing check on the host.  Recovery: recover.hip.
// With ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT (CellChallengeMode::leaf) the challenge is the leaf-hashed one instead (verify_host.hpp:
// CellLeafTranscript): one SHA-256 per cell on the GPU (k_sha256.hip), the root over the digests on the host.
#include "engine_internal.hpp"
#include "curve29.hpp"
#include "host_pairing.hpp"
#include "vm_search.hpp"

namespace kzg {

static_assert(INPUT_VALID == OK && INPUT_INVALID == ERR_INPUT && INPUT_MAX_CELLS == MAX_CELLS_PER_VERIFICATION, "verify_host.hpp states engine.hpp's codes");

void Engine::init_verifier() {
    launch::init_attributes_verify();
    pairing::init();
    // G2 points of the verification key: [1]_2 = g2_monomial[0], [tau^64]_2 = g2_monomial[64]
    const unsigned char* g2 = setup_->g2.data();
    pairing::G2Affine gen, tau;
    if (!pairing::g2_decompress(gen, g2) || !pairing::g2_decompress(tau, g2 + 96 * CELL_LEN))
        throw std::runtime_error("trusted setup: G2 point failed to decompress");
    g2_tau_ = std::make_shared<pairing::G2Prepared>(pairing::prepare(tau));
    g2_neg_gen_ = std::make_shared<pairing::G2Prepared>(pairing::prepare(pairing::g2_neg(gen)));
    pairing::G2Affine tau1;
    if (!pairing::g2_decompress(tau1, g2 + 96)) throw std::runtime_error("trusted setup: [tau]_2 failed to decompress");
    g2_tau1_ = std::make_shared<pairing::G2Prepared>(pairing::prepare(tau1));
    if (!setup_->embedded && !primary_) {
        // A tau inside the evaluation domain (tau^8192 = 1; tau = 1 is the plain case) makes tau^64 equal to h_k^64 for one of the 128
        // cosets: the key [tau^64 - h_k^64]_2 that cell k's opening is checked against is the point at infinity and every "proof"
        // for that cell verifies.  tau^8192 = 1 <=> tau^4096 = +-1 <=> e([tau^4095]_1, [tau]_2) = e([1]_1, [1]_2)^(+-1): two pairing
        // checks on points the context holds anyway.  No honest setup is in this case; never wrong answers, so it is refused.
        G1Affine P[2];
        HIPCK(hipMemcpy(&P[0], (const G1Affine*)d_srs_ + (N_BLOB - 1), sizeof(G1Affine), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(&P[1], (const G1Affine*)d_srs_, sizeof(G1Affine), hipMemcpyDeviceToHost));
        const pairing::G2Prepared gen_p = pairing::prepare(gen);
        const pairing::G2Prepared* minus[2] = {g2_tau1_.get(), g2_neg_gen_.get()};  // tau^4096 = 1
        const pairing::G2Prepared* plus[2] = {g2_tau1_.get(), &gen_p};              // tau^4096 = -1
        if (pairing::product_is_one(P, minus, 2) || pairing::product_is_one(P, plus, 2))
            throw std::runtime_error("degenerate trusted setup: tau is a root of unity of the evaluation domain (tau^8192 = 1), so a derived "
                                     "verification base [tau^64 - h^64]_2 is the point at infinity");
    }
    // the prepared keys and the Frobenius constants in HBM: from the SAME objects the host's checks use (vm_search.hpp)
    {
        const pairing::G2Prepared* keys[3] = {g2_tau_.get(), g2_neg_gen_.get(), g2_tau1_.get()};
        bool all = true;
        for (const pairing::G2Prepared* k : keys) all = all && !k->inf && (int)k->lines.size() == pairing::MILLER_LINES;
        gpu_pairing_min_ = knobs_.gpu_pairing_min >= 0 ? knobs_.gpu_pairing_min : vm::GPU_PAIRING_MIN_DEFAULT;
        if (!all) gpu_pairing_min_ = 0;
        if (all) {
            constexpr size_t KEY = (size_t)pairing::MILLER_LINES * sizeof(pairing::Line);
            std::vector<uint8_t> img(3 * KEY + sizeof(pairing::FrobConsts));
            for (int k = 0; k < 3; k++) memcpy(img.data() + (size_t)k * KEY, keys[k]->lines.data(), KEY);
            memcpy(img.data() + 3 * KEY, &pairing::frob_consts(), sizeof(pairing::FrobConsts));
            HIPCK(hipMalloc(&d_pairing_, img.size()));
            HIPCK(hipMemcpy(d_pairing_, img.data(), img.size(), hipMemcpyHostToDevice));
        }
    }
    // coset shift tables 7^i, 7^-i
    std::vector<Fr> c(N_EXT), ci(N_EXT);
    Fr g = fr_u64(7), gi = inv(g);
    c[0] = ci[0] = one<FrParams>();
    for (int i = 1; i < N_EXT; i++) { c[i] = mul(c[i - 1], g); ci[i] = mul(ci[i - 1], gi); }
    HIPCK(hipMalloc(&d_coset_, N_EXT * sizeof(Fr)));
    HIPCK(hipMalloc(&d_coset_inv_, N_EXT * sizeof(Fr)));
    HIPCK(hipMemcpy(d_coset_, c.data(), N_EXT * sizeof(Fr), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(d_coset_inv_, ci.data(), N_EXT * sizeof(Fr), hipMemcpyHostToDevice));
    inv64_ = to8(inv(fr_u64(64)));
    n_inv8192_ = to8(inv(fr_u64(N_EXT)));
}

namespace {

// Where one call's arrays lie.  Device arena: [inputs, uploaded in ONE copy | device only]; the pinned slab holds the same inputs
// and, behind them, the read-backs.  n cells of this shard, m unique commitments of the batch.
struct Layout {
    const int n, m;
    const bool shifted;  // the byte-shifted lincombs (k_verify.hip): point copies and per-cell interpolation polynomials are built behind the hash
    const bool leaf;     // the leaf-hashed challenge: n x 32 digest bytes on the device and, read back, in the pinned slab
    const size_t npts = (size_t)n + m + 64;  // one point array [proofs n | commitments m | 64 SRS points] so that the second lincomb is a single MSM
    const int ib = n < 256 ? n : 256;
    const size_t sz_c = (size_t)m * 48, sz_p = (size_t)n * 48, sz_cells = (size_t)n * BYTES_PER_CELL, sz_i = (size_t)n * sizeof(int);
    Carve d;  // (members are initialised in the order they stand here)
    const size_t off_c = d.take(sz_c), off_p = d.take(sz_p), off_cells = d.take(sz_cells), off_idx = d.take(sz_i), off_row = d.take(sz_i), in_bytes = d.end;
    Carve h = d;  // pinned read-back area behind the inputs: statuses (m + n + 1 ints) and room for the two result points
    const size_t n_status = (size_t)m + n + 1, off_hst = h.take(n_status * sizeof(int)), off_hleaf = h.take(leaf ? (size_t)n * 32 : 0),
                 pin_bytes = (h.take(256), h.end);
    const size_t off_pts = d.take(npts * sizeof(G1Affine)), off_evals = d.take((size_t)n * CELL_LEN * sizeof(Fr)), off_stc = d.take((size_t)m * sizeof(int)),
                 off_stp = d.take(sz_i), off_ste = d.take(sizeof(int)), off_rp = d.take((size_t)n * sizeof(Fr)), off_s1 = d.take((size_t)n * sizeof(Fr)),
                 off_sB = d.take(npts * sizeof(Fr)), off_part = d.take((size_t)ib * 64 * sizeof(Fr)),
                 off_ws = d.take(shifted ? launch::pip_shift_workspace_bytes((int)npts) : launch::pip_workspace_bytes((int)npts)),
                 off_coef = d.take(shifted ? (size_t)n * CELL_LEN * sizeof(Fr) : 0),
                 off_out = d.take(512),  // two affine points, or two Jacobian sums (shifted form)
                 off_leaf = d.take(leaf ? (size_t)n * 32 : 0),
                 dev_bytes = d.end;
    Layout(int n_, int m_, bool shifted_, bool leaf_ = false) : n(n_), m(m_), shifted(shifted_), leaf(leaf_) {}
};

// the end of a staging task, seen from the frame whose locals the task uses
struct StageDone {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    std::exception_ptr error;  // the task's; read after wait()
    void wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [this] { return done; }); }
    void signal() { std::lock_guard<std::mutex> lk(mu); done = true; cv.notify_all(); }
};

// One call of Engine::verify_cells_partial: what its steps share, as plain values (the member function fills them in).
struct CellPass {
    const Layout L;
    explicit CellPass(const Layout& l) : L(l) {}
    int k0 = 0;  // this shard: cells k0 .. k0 + n, global exponents r^(k0 + k)
    int dev = 0;
    hipStream_t st = nullptr;
    uint8_t *hb = nullptr, *db = nullptr;  // pinned slab, device arena
    // the caller's batch
    const uint8_t* const* uniq = nullptr;
    const int* row = nullptr;
    const uint64_t* cell_indices = nullptr;
    const uint8_t* const* cells = nullptr;
    const uint8_t* const* proofs = nullptr;
    // device-resident form (src_cells != null): cells and proofs move inside HBM; `cells` is their pinned mirror, arriving in chunks
    const uint8_t *src_cells = nullptr, *src_proofs = nullptr;
    hipEvent_t* chunk_events = nullptr;
    int chunk_cells = 0, n_chunks = 0;
    // the engine's constants
    const void *d_srs = nullptr, *d_w8192 = nullptr;
    Fp12w beta;
    Fr8 inv64;
    hipStream_t side = nullptr;  // round 3's form (ETH_KZG_AMD_VERIFY_SIDE_STREAM=1): the subgroup tests on this second stream; null: one stream
    hipEvent_t decoded = nullptr, checked = nullptr;
    // leaf-hashed challenge (L.leaf): the leaves are hashed on leaf_st behind `uploaded`, next to the decoding on st; `leaves` is
    // recorded behind the read-back of their digests
    hipStream_t leaf_st = nullptr;
    hipEvent_t uploaded = nullptr, leaves = nullptr;

    int* h_status() const { return (int*)(hb + L.off_hst); }  // pinned: [commitments m | proofs n | cells 1]; the read-backs do not block
    G1Affine* d_proofs_aff() const { return (G1Affine*)(db + L.off_pts); }
    G1Affine* d_commitments_aff() const { return d_proofs_aff() + L.n; }

    // ---- staging, upload and deserialisation: the pool task, while the calling thread hashes the transcript
    void stage_and_decode() const {
        const int n = L.n, m = L.m;
        HIPCK(hipSetDevice(dev));
        uint8_t *hc = hb + L.off_c, *hp = hb + L.off_p, *hcells = hb + L.off_cells;
        int *hidx = (int*)(hb + L.off_idx), *hrow = (int*)(hb + L.off_row);
        // gather the caller's scattered buffers into ONE pinned host slab, one async copy to a persistent device arena
        for (int i = 0; i < m; i++) memcpy(hc + (size_t)i * 48, uniq[i], 48);
        for (int k = 0; k < n; k++) {
            if (!src_cells) {
                memcpy(hp + (size_t)k * 48, proofs[k0 + k], 48);
                memcpy(hcells + (size_t)k * BYTES_PER_CELL, cells[k0 + k], BYTES_PER_CELL);
            }
            hidx[k] = (int)cell_indices[k0 + k];
            hrow[k] = row[k0 + k];
        }
        int *d_stc = (int*)(db + L.off_stc), *d_stp = (int*)(db + L.off_stp), *d_ste = (int*)(db + L.off_ste);
        // stale contents of the persistent arena must fail closed: poison every status word and the result slot
        // (device side and pinned read-back side) before anything is launched
        memset(h_status(), 0xff, L.n_status * sizeof(int));
        HIPCK(hipMemsetAsync(d_stc, 0xff, (size_t)m * sizeof(int), st));
        HIPCK(hipMemsetAsync(d_stp, 0xff, (size_t)n * sizeof(int), st));
        HIPCK(hipMemsetAsync(db + L.off_out, 0xff, 512, st));
        if (!src_cells) {
            HIPCK(hipMemcpyAsync(db, hb, L.in_bytes, hipMemcpyHostToDevice, st));
        } else {  // device-resident form: only the small host-made parts go up; cells and proofs move inside HBM
            HIPCK(hipMemcpyAsync(db + L.off_c, hb + L.off_c, L.sz_c, hipMemcpyHostToDevice, st));
            HIPCK(hipMemcpyAsync(db + L.off_idx, hb + L.off_idx, L.in_bytes - L.off_idx, hipMemcpyHostToDevice, st));
            HIPCK(hipMemcpyAsync(db + L.off_p, src_proofs + (size_t)k0 * 48, L.sz_p, hipMemcpyDeviceToDevice, st));
            HIPCK(hipMemcpyAsync(db + L.off_cells, src_cells + (size_t)k0 * BYTES_PER_CELL, L.sz_cells, hipMemcpyDeviceToDevice, st));
        }
        HIPCK(hipMemsetAsync(d_ste, 0, sizeof(int), st));
        if (L.leaf) {
            // the leaves straight out of the arena (every offset of it is a multiple of 256: the kernel's 16-byte loads), on a stream of
            // their own: a wave per 64 cells for 35 dependent compressions leaves the chip to the decoding below, and the digests are
            // down and the root hashed while that runs.  (A call that goes on to use r has waited for `leaves` on the host: its work on
            // leaf_st is over before the arena is touched again.)
            uint8_t* d_leaf = db + L.off_leaf;
            HIPCK(hipEventRecord(uploaded, st));
            HIPCK(hipStreamWaitEvent(leaf_st, uploaded, 0));
            launch::sha256_cell_leaves(n, db + L.off_c, (const int*)(db + L.off_row), (const int*)(db + L.off_idx), db + L.off_p, db + L.off_cells, d_leaf, leaf_st);
            HIPCK(hipMemcpyAsync(hb + L.off_hleaf, d_leaf, (size_t)n * 32, hipMemcpyDeviceToHost, leaf_st));
            HIPCK(hipEventRecord(leaves, leaf_st));
        }
        // deserialisation with on-curve + subgroup checks (serialization/src/lib.rs:69-99), on the GPU
        const uint8_t *d_cb = db + L.off_c, *d_pb = db + L.off_p, *d_cellb = db + L.off_cells;
        G1Affine *d_prf_p = d_proofs_aff(), *d_comm_p = d_commitments_aff();
        void* d_evals = db + L.off_evals;
        if (L.shifted) {
            // decode on this stream; the subgroup tests (126 dependent doublings per point) next to everything that needs only
            // the coordinates and not the challenge: the byte-shifted point copies (120 dependent doublings per point) and
            // the per-cell interpolation polynomials
            launch::g1_decode2(d_pb, d_prf_p, d_stp, n, d_cb, d_comm_p, d_stc, m, beta, st);
            launch::copy_affine(d_srs, d_comm_p + m, 64, st);  // vk.g1s: the first 64 SRS points (verification_key.rs:66-70)
            launch::cells_to_fr(d_cellb, d_evals, nullptr, d_ste, nullptr, nullptr, n, st);
            if (side) {
                HIPCK(hipEventRecord(decoded, st));
                HIPCK(hipStreamWaitEvent(side, decoded, 0));
                launch::g1_subgroup2(d_prf_p, d_stp, n, d_comm_p, d_stc, m, beta, side);
                HIPCK(hipEventRecord(checked, side));
                launch::pip_shift_prepare(d_prf_p, (int)L.npts, (int)L.npts, db + L.off_ws, beta, st);
            } else {
                launch::pip_shift_prepare_and_subgroup(d_prf_p, (int)L.npts, (int)L.npts, db + L.off_ws, d_prf_p, d_stp, n, d_comm_p, d_stc, m, beta, st);
            }
            launch::interp_cells(d_evals, (const int*)(db + L.off_idx), d_w8192, inv64, db + L.off_coef, n, st);
            if (side) HIPCK(hipStreamWaitEvent(st, checked, 0));
        } else {
            launch::g1_decompress2(d_pb, d_prf_p, d_stp, n, d_cb, d_comm_p, d_stc, m, beta, st);
            launch::copy_affine(d_srs, d_comm_p + m, 64, st);  // vk.g1s: the first 64 SRS points (verification_key.rs:66-70)
            launch::cells_to_fr(d_cellb, d_evals, nullptr, d_ste, nullptr, nullptr, n, st);
        }
        int* stc = h_status();
        HIPCK(hipMemcpyAsync(stc, d_stc, m * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(stc + m, d_stp, n * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(stc + m + n, d_ste, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCK(hipGetLastError());  // launch failures are per thread: this thread's would be lost with it
    }

    // ---- the Fiat-Shamir challenge, hashed straight from the caller's buffers while the GPU decompresses.  The transcript always
    // covers the whole batch (n_all cells), whatever the shard.
    Fr challenge(int n_all, uint8_t* digest_out) const {
        CellBatchTranscript t(L.m, n_all, uniq);
        int chunks_in = 0;  // (device-resident form) chunks of the cells' host mirror that have arrived
        for (int k = 0; k < n_all; k++) {
            while (chunks_in < n_chunks && k >= chunks_in * chunk_cells) HIPCK(hipEventSynchronize(chunk_events[chunks_in++]));
            t.absorb(row[k], cell_indices[k], cells[k], proofs[k]);
        }
        const Fr r = t.finish();
        if (digest_out) memcpy(digest_out, t.digest(), 32);
        return r;
    }
    // ---- the leaf-hashed challenge (the whole batch is this pass: L.n cells): the root over the leaf digests the GPU hashed.  Called
    // once stage_and_decode has returned (the event is recorded); the decoding kernels are still running.
    Fr challenge_leaf(uint8_t* digest_out, uint8_t* leaves_out) const {
        HIPCK(hipEventSynchronize(leaves));
        const uint8_t* dig = hb + L.off_hleaf;
        CellLeafTranscript t;
        const Fr r = t.root((uint64_t)L.n, dig);
        if (digest_out) memcpy(digest_out, t.digest(), 32);
        if (leaves_out) memcpy(leaves_out, dig, (size_t)L.n * 32);
        return r;
    }

    // ---- what the decoding found, in the order of the reference: commitments, proofs, cells
    int read_verdicts() const {
        const int *stc = h_status(), *stp = stc + L.m, *ste = stp + L.n;
        for (int i = 0; i < L.m; i++) if (stc[i]) return ERR_G1;
        for (int i = 0; i < L.n; i++) if (stp[i]) return ERR_G1;
        return *ste ? ERR_SCALAR : OK;
    }

    // ---- the scalars from the challenge, then the four lincombs (verifier.rs:186,200,224,235) as two bucket MSMs over the shared
    // point array:   out[0] = sum r^k pi_k;   out[1] = sum r^k h^64 pi_k + sum w_row C_row - commit(interpolation poly)
    void scalars_and_lincombs(const Fr& r, G1Affine* out) const {
        const int n = L.n, m = L.m;
        Fr8 tab[24];
        Fr cur = r;
        for (int i = 0; i < 24; i++) { tab[i] = to8(cur); cur = sqr(cur); }
        const int* d_idx = (const int*)(db + L.off_idx);
        void *d_rp = db + L.off_rp, *d_s1 = db + L.off_s1, *d_sB = db + L.off_sB, *d_part = db + L.off_part;
        Fr* d_s2 = (Fr*)d_sB;
        Fr* d_w = d_s2 + n;
        Fr* d_interp = d_w + m;
        launch::verify_scalars(tab, k0, d_idx, d_w8192, d_rp, d_s1, d_s2, n, st);
        launch::verify_weights(d_rp, (const int*)(db + L.off_row), d_w, n, m, st);
        if (L.shifted) launch::interp_sum(db + L.off_coef, d_rp, d_part, L.ib, d_interp, n, st);
        else launch::interp(db + L.off_evals, d_idx, d_rp, d_w8192, inv64, d_part, L.ib, d_interp, n, st);
        void *d_ws = db + L.off_ws, *d_out = db + L.off_out;
        if (L.shifted) {
            launch::msm_pippenger2_shifted(d_s1, n, d_sB, n + m + 64, (int)L.npts, d_ws, d_out, st);
            JacQ sums[2];
            HIPCK(hipMemcpyAsync(sums, d_out, sizeof sums, hipMemcpyDeviceToHost, st));
            SYNC_CHECKED(st);
            for (int i = 0; i < 2; i++) {
                if (sums[i].x.v[0] == 0xffffffffu && sums[i].z.v[0] == 0xffffffffu) throw std::runtime_error("verification MSM left no result");
                out[i] = to_affine(jac_from_jacq(sums[i]));
            }
        } else {
            launch::msm_pippenger2(d_proofs_aff(), d_s1, n, d_sB, n + m + 64, d_ws, d_out, beta, st);
            HIPCK(hipMemcpyAsync(out, d_out, 2 * sizeof(G1Affine), hipMemcpyDeviceToHost, st));
            SYNC_CHECKED(st);
        }
        for (int i = 0; i < 2; i++)  // the poison pattern (or anything else that is not a reduced coordinate) is a device failure
            if (out[i].x.v[11] > FpParams::MOD[11] || out[i].y.v[11] > FpParams::MOD[11]) throw std::runtime_error("verification MSM left no result");
    }
};

}  // namespace

// The verification equation is linear in the cells: with the challenge r taken over the WHOLE batch, the two G1
// pairing inputs are sums of per-cell terms, so a shard [lo, hi) of the cell list yields two partial points and the
// partials of all shards add up to the pairing inputs of the full batch.
// `out` receives the two partial points; *empty is set when the batch has no cells at all (verifier.rs:90-93).
int Engine::verify_cells_partial(uint64_t n_commitments, const uint8_t* const* commitments, uint64_t n_indices,
                                 const uint64_t* cell_indices, uint64_t n_cells, const uint8_t* const* cells,
                                 uint64_t n_proofs, const uint8_t* const* proofs, uint64_t lo, uint64_t hi,
                                 G1Affine* out, bool* empty, const VerifyDeviceSource* dsrc, VerifyScratch* vs, const CellChallengeMode* mode) {
    const bool leaf = mode && mode->leaf;
    *empty = false;
    out[0] = out[1] = aff_inf();
    if (validate_cell_batch(n_commitments, n_indices, n_cells, n_proofs, cell_indices) != OK) return ERR_INPUT;
    if (lo > hi || hi > n_cells) return ERR_INPUT;
    if (leaf && (lo != 0 || hi != n_cells || vs)) return ERR_INPUT;  // the leaf-hashed challenge is for whole batches under mu_ (the sharded forms keep the reference's)
    const int n_all = (int)n_cells;
    if (n_all == 0) { *empty = true; return OK; }  // verifier.rs:90-93
    if (lo == hi) return OK;                       // an empty shard contributes the identity twice
    std::unique_lock<std::recursive_mutex> lk(mu_, std::defer_lock);
    try {
        std::vector<const uint8_t*> uniq;
        std::vector<int> row;
        dedup_commitments(n_commitments, commitments, uniq, row);  // (before the lock: it is the caller's data, and concurrent callers overlap here)
        if (!vs) lk.lock();  // the engine's own scratch under its lock, or a pass slot's (its holder called)
        TraceLap lap{knobs_.trace, "verify"};
        HIPCK(hipSetDevice(dev_));
        hipStream_t st = vs ? vs->stream : stream_;
        const int n = (int)(hi - lo);
        const Layout L(n, (int)uniq.size(), n >= pip_shift_min_, leaf);
        grow_device(vs ? vs->dev : v_dev_, vs ? vs->dev_cap : v_dev_cap_, L.dev_bytes, st);  // (no per-call hipMalloc)
        grow_pinned(vs ? vs->pin : v_pin_, vs ? vs->pin_cap : v_pin_cap_, L.pin_bytes);
        CellPass pass(L);
        pass.k0 = (int)lo; pass.dev = dev_; pass.st = st;
        pass.hb = vs ? vs->pin : v_pin_; pass.db = (uint8_t*)(vs ? vs->dev : v_dev_);
        pass.uniq = uniq.data(); pass.row = row.data(); pass.cell_indices = cell_indices; pass.cells = cells; pass.proofs = proofs;
        if (dsrc) {
            pass.src_cells = dsrc->d_cells; pass.src_proofs = dsrc->d_proofs;
            pass.chunk_events = dsrc->chunk_events; pass.chunk_cells = dsrc->chunk_cells; pass.n_chunks = dsrc->n_chunks;
        }
        pass.d_srs = d_srs_; pass.d_w8192 = d_w8192_; pass.beta = beta_; pass.inv64 = inv64_;
        if (v_two_streams_ && !vs) pass.side = v_side_;
        pass.decoded = v_decoded_; pass.checked = v_checked_; pass.leaves = v_leaves_;
        pass.leaf_st = v_leaf_stream_; pass.uploaded = v_uploaded_;
        // (a worker of the engine's small persistent pool: starting and joining a fresh thread per call was 50-100 us of a 3.3 ms call)
        std::call_once(stage_pool_once_, [this] { stage_pool_.reset(new HostPool(primary_ ? 1 : 4, [d = dev_] { (void)hipSetDevice(d); })); });
        StageDone staged;
        stage_pool_->submit([&pass, &staged]() {
            struct Signal { StageDone& s; ~Signal() { s.signal(); } } signal{staged};
            try {
                pass.stage_and_decode();
            } catch (...) {
                staged.error = std::current_exception();
            }
        });
        struct Joiner { StageDone& s; ~Joiner() { s.wait(); } } joiner{staged};  // whatever happens below, the task has left this frame first
        Fr r;
        if (leaf) {
            staged.wait();
            if (staged.error) std::rethrow_exception(staged.error);
            lap("stage + enqueue (host)");
            r = pass.challenge_leaf(mode->digest_out, mode->leaves_out);
            lap("leaf hashes (GPU) + root (host)");
        } else {
            r = pass.challenge(n_all, mode ? mode->digest_out : nullptr);
            lap("sha256 transcript (host)");
            staged.wait();
            if (staged.error) std::rethrow_exception(staged.error);
        }
        SYNC_CHECKED(st);
        lap("wait decompress/deserialise");
        if (leaf && mode->leaves_out) return OK;  // (the stage hook of the leaf kernel: the digests are what it asked for)
        if (const int verdict = pass.read_verdicts()) return verdict;
        pass.scalars_and_lincombs(r, out);
        lap("scalars+interp+lincombs (GPU)");
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// pairing check e(sum r^k pi_k, [tau^64]_2) * e(C - I + weighted proofs, -[1]_2) == 1 (verifier.rs:242-259)
bool Engine::verify_cells_pairing(const G1Affine* pts) const {
    const pairing::G2Prepared* q[2] = {g2_tau_.get(), g2_neg_gen_.get()};
    return pairing::product_is_one(pts, q, 2);
}

// A single verification waits for its pairing check on the calling thread (0.85 ms of 2.8).  The two Miller loops are
// independent, so the second one goes to a thread of the staging pool (idle by now: its staging task finished before the
// challenge) and the values meet in front of the one final exponentiation: 63 squarings + 68 line products per thread instead
// of 63 + 136 on one.  Whoever gets to the second loop first computes it -- a busy pool costs nothing.
bool Engine::verify_cells_pairing_split(const G1Affine* pts) {
    if (!stage_pool_) return verify_cells_pairing(pts);
    struct Shared {
        pairing::Fp12 f;
        G1Affine p;
        std::atomic<int> claimed{0}, done{0};
    };
    auto sh = std::make_shared<Shared>();
    sh->p = pts[1];
    const pairing::G2Prepared* q1 = g2_neg_gen_.get();
    stage_pool_->submit([sh, q1] {
        if (sh->claimed.exchange(1, std::memory_order_acq_rel)) return;
        sh->f = pairing::miller_loop(sh->p, *q1);
        sh->done.store(1, std::memory_order_release);
    });
    const pairing::Fp12 f0 = pairing::miller_loop(pts[0], *g2_tau_);
    if (!sh->claimed.exchange(1, std::memory_order_acq_rel)) {
        sh->f = pairing::miller_loop(sh->p, *q1);
    } else {
        while (!sh->done.load(std::memory_order_acquire)) std::this_thread::yield();
    }
    return pairing::final_exponentiation_is_one(pairing::fp12_mul(f0, sh->f));
}

// Device-resident form of the same check: the four flat arrays already sit in this GPU's HBM (cells straight from a prover or
// recovery call, for instance) and STAY there for the GPU's part: decoding, subgroup tests, shifted copies and interpolation
// read them after a device-to-device copy into the arena, at once.  What has to come down is what the Fiat-Shamir transcript
// hashes -- a sequential SHA-256 over every byte, which belongs on a host core (2 cycles per byte with SHA-NI: 7.2 ms for
// config 3's 17.6 MB, the floor of this call): commitments, indices and proofs first (0.9 MB; the host de-duplicates the
// commitments), then the cells in eight chunks that the hash consumes as they land (PCIe delivers 20x faster than it reads).
// Round 3 copied everything down, gathered it on the host and uploaded it again.
// With the leaf-hashed challenge (mode->leaf) that floor is gone: the leaves are hashed in HBM and neither cells nor proofs come down
// (verify_cells_partial_device: its first branch).
int Engine::verify_cell_kzg_proof_batch_device(uint64_t n, const uint8_t* d_commitments, const uint64_t* d_cell_indices,
                                               const uint8_t* d_cells, const uint8_t* d_proofs, int* verified, hipStream_t user_stream,
                                               const CellChallengeMode* mode) {
    *verified = 0;
    if (n == 0) { *verified = 1; return OK; }  // verifier.rs:90-93
    if (n > MAX_CELLS_PER_VERIFICATION) return ERR_INPUT;
    std::lock_guard<std::recursive_mutex> lk(mu_);  // the pinned mirror is the context's (grow-only, reused by every call)
    G1Affine pts[2];
    bool empty = false;
    const int rc = verify_cells_partial_device(n, d_commitments, d_cell_indices, d_cells, d_proofs, 0, n, pts, &empty, user_stream, mode);
    if (rc) return rc;
    *verified = (empty || verify_cells_pairing_split(pts)) ? 1 : 0;
    return OK;
}

// 1 <= n <= MAX_CELLS_PER_VERIFICATION; the two partial points of the cells [lo, hi) as verify_cells_partial leaves them.
// The caller holds mu_ (the product call above through its pairing check; the test hook for the call).
int Engine::verify_cells_partial_device(uint64_t n, const uint8_t* d_commitments, const uint64_t* d_cell_indices, const uint8_t* d_cells,
                                        const uint8_t* d_proofs, uint64_t lo, uint64_t hi, G1Affine* pts, bool* empty, hipStream_t user_stream,
                                        const CellChallengeMode* mode) {
    int rc = OK;
    if (mode && mode->leaf) {
        // Leaf-hashed challenge: nothing the hash reads has to come down.  Commitments and indices do (0.5 MB for 8192 cells), for
        // validation and de-duplication; the proofs and the cells are hashed, cell by cell, where the device-to-device copy puts them.
        try {
            std::vector<const uint8_t*> cp(n);
            HIPCK(hipSetDevice(dev_));
            const size_t sz_c = n * 48, sz_i = n * sizeof(uint64_t);
            grow_pinned(vd_pin_, vd_pin_cap_, sz_c + sz_i);
            uint8_t *pin_c = vd_pin_, *pin_i = vd_pin_ + sz_c;
            hipStream_t st = stream_;
            order_behind(st, user_stream, v_decoded_);
            HIPCK(hipMemcpyAsync(pin_c, d_commitments, sz_c, hipMemcpyDeviceToHost, st));
            HIPCK(hipMemcpyAsync(pin_i, d_cell_indices, sz_i, hipMemcpyDeviceToHost, st));
            HIPCK(hipStreamSynchronize(st));
            for (uint64_t k = 0; k < n; k++) cp[k] = pin_c + k * 48;
            const VerifyDeviceSource src{d_cells, d_proofs, nullptr, 0, 0};
            return verify_cells_partial(n, cp.data(), n, reinterpret_cast<const uint64_t*>(pin_i), n, nullptr, n, nullptr, lo, hi, pts, empty, &src, nullptr, mode);
        } catch (const std::exception& e) {
            set_error(e);
            return ERR_DEVICE;
        }
    }
    try {
        std::vector<const uint8_t*> cp(n), lp(n), pp(n);  // inside the try: a bogus n must not unwind through the C ABI
        HIPCK(hipSetDevice(dev_));
        const size_t sz_c = n * 48, sz_i = n * sizeof(uint64_t), sz_l = n * (size_t)BYTES_PER_CELL, sz_p = n * 48;
        const size_t need = sz_c + sz_i + sz_l + sz_p;
        grow_pinned(vd_pin_, vd_pin_cap_, need);
        for (hipEvent_t& e : vd_events_)
            if (!e) HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        uint8_t* pin = vd_pin_;
        uint8_t *pin_c = pin, *pin_i = pin + sz_c, *pin_p = pin + sz_c + sz_i, *pin_l = pin + sz_c + sz_i + sz_p;
        hipStream_t st = stream_;
        order_behind(st, user_stream, v_decoded_);
        HIPCK(hipMemcpyAsync(pin_c, d_commitments, sz_c, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(pin_i, d_cell_indices, sz_i, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(pin_p, d_proofs, sz_p, hipMemcpyDeviceToHost, st));
        HIPCK(hipEventRecord(v_checked_, st));
        const int n_chunks = n >= 64 * VD_CHUNKS ? VD_CHUNKS : 1, chunk_cells = (int)((n + n_chunks - 1) / n_chunks);
        for (int j = 0; j < n_chunks; j++) {
            const size_t c0 = (size_t)j * chunk_cells, c1 = std::min<size_t>(n, c0 + chunk_cells);
            if (c1 > c0) HIPCK(hipMemcpyAsync(pin_l + c0 * BYTES_PER_CELL, d_cells + c0 * BYTES_PER_CELL, (c1 - c0) * BYTES_PER_CELL, hipMemcpyDeviceToHost, st));
            HIPCK(hipEventRecord(vd_events_[j], st));
        }
        HIPCK(hipEventSynchronize(v_checked_));  // commitments, indices, proofs are down: validation and de-duplication can start
        for (uint64_t k = 0; k < n; k++) {
            cp[k] = pin_c + k * 48;
            lp[k] = pin_l + k * (size_t)BYTES_PER_CELL;
            pp[k] = pin_p + k * 48;
        }
        const VerifyDeviceSource src{d_cells, d_proofs, vd_events_, chunk_cells, n_chunks};
        rc = verify_cells_partial(n, cp.data(), n, reinterpret_cast<const uint64_t*>(pin_i), n, lp.data(), n, pp.data(), lo, hi, pts, empty, &src, nullptr, mode);
        if (rc != OK || lo == hi) (void)hipStreamSynchronize(st);  // (an early return, error or empty range: the copies into the mirror must not outlive the call)
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return rc;
}

int Engine::verify_cell_kzg_proof_batch_host(uint64_t n_commitments, const uint8_t* const* commitments, uint64_t n_indices,
                                             const uint64_t* cell_indices, uint64_t n_cells, const uint8_t* const* cells,
                                             uint64_t n_proofs, const uint8_t* const* proofs, int* verified, const CellChallengeMode* mode) {
    *verified = 0;
    G1Affine pts[2];
    bool empty = false;
    int st = verify_cells_partial(n_commitments, commitments, n_indices, cell_indices, n_cells, cells, n_proofs, proofs, 0,
                                  n_cells, pts, &empty, nullptr, nullptr, mode);
    if (st) return st;
    TraceLap lap{knobs_.trace, "verify"};
    *verified = (empty || verify_cells_pairing_split(pts)) ? 1 : 0;
    lap("pairing check (host)");
    return OK;
}

// Sharded form, step 1: this rank's cells [lo, hi) of the batch -> 96 bytes (two compressed G1 partial sums).
int Engine::verify_cell_kzg_proof_batch_partial_host(uint64_t n_commitments, const uint8_t* const* commitments,
                                                     uint64_t n_indices, const uint64_t* cell_indices, uint64_t n_cells,
                                                     const uint8_t* const* cells, uint64_t n_proofs,
                                                     const uint8_t* const* proofs, uint64_t lo, uint64_t hi, uint8_t* out96) {
    G1Affine pts[2];
    bool empty = false;
    int st = verify_cells_partial(n_commitments, commitments, n_indices, cell_indices, n_cells, cells, n_proofs, proofs, lo, hi,
                                  pts, &empty);
    if (st) return st;
    g1_compress(out96, pts[0]);
    g1_compress(out96 + 48, pts[1]);
    return OK;
}

// Sharded form, step 2: add the partials of all shards (group addition is not an RCCL reduction, so the gathered
// 96-byte records are summed on the host) and run the one pairing check.
int Engine::verify_cell_kzg_proof_batch_combine_host(uint64_t n_partials, const uint8_t* partials96, int* verified) {
    *verified = 0;
    G1Jac acc[2] = {jac_inf(), jac_inf()};
    for (uint64_t i = 0; i < n_partials; i++)
        for (int j = 0; j < 2; j++) {
            G1Affine a;
            if (g1_decompress(a, partials96 + i * 96 + 48 * j) != 0) return ERR_G1;
            acc[j] = add_mixed(acc[j], a);
        }
    G1Affine pts[2] = {to_affine(acc[0]), to_affine(acc[1])};
    // no cells anywhere => both sums are the identity and the product of pairings is 1, as the reference's early return
    *verified = verify_cells_pairing(pts) ? 1 : 0;
    return OK;
}

}  // namespace kzg
