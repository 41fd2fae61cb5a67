// eth_kzg_amd_verify_cell_kzg_proof_batch_many: MANY independent verify_cell_kzg_proof_batch problems in one call.
// Reference semantics per problem: DASContext::verify_cell_kzg_proof_batch (crates/eip7594/src/verifier.rs:72-164) ->
// FK20Verifier::verify_multi_opening (crates/cryptography/kzg_multi_open/src/fk20/verifier.rs:129-260); the reference gets
// its throughput by verifying from many threads on one context (bindings/node/src/lib.rs:92-299,
// crates/cryptography/bls12_381/src/lib.rs:45-50).  Here the problems of a call share every GPU launch:
//   host threads : validation + de-duplication per problem, staging into one pinned slab, one SHA-256 transcript per problem
//                  (in parallel, behind the GPU's decoding; a persistent pool), then ONE 2-pairing check per pass: the problems' two
//                  G1 sums are folded on the GPU with 127-bit weights derived from all the challenges; in a pass whose folded check
//                  fails (some proof is wrong) the wrong problems are SEARCHED by folding sub-ranges of the resident weighted sums,
//                  one pairing per probe ($ETH_KZG_AMD_VM_SEARCH=0: re-checked one by one; $ETH_KZG_AMD_VM_FOLD=0: never folded)
//   GPU          : decode + subgroup-check all points, decode all cells, per-cell interpolation (challenge-free: behind the
//                  hashes), then per-problem scalars / weights / interpolation sums, ONE LANE PER SCALAR MULTIPLICATION
//                  (k_verify_many.hip), the 64-term interpolation commitments from the commitment window table, per-problem sums;
//                  small passes (concurrent single calls combined) take a short-chain form: everything after the challenge in
//                  one launch, no fold
// Three pass slots, each with its own lock, device arena and pinned slab, on the streams of the prover's three work sets (HIP maps
// a process's streams onto four hardware queues): passes run side by side, a large call is cut into three concurrent parts, and a
// "pass" of one problem is the single path on the slot.  Nothing here takes the context's big lock.
// One pass, two sources, two challenge modes (engine.hpp: VerifyManyInput).  Sources: the caller's pointer lists, gathered into the
// pinned slab and uploaded; or flat arrays in HBM plus cell_starts, whose proofs and cells go device-to-device into the arena while
// commitments and indices come down for validation and de-duplication.  Challenges: the reference's transcript on the host threads; or
// the leaf-hashed challenge of each problem alone (verify_host.hpp: CellLeafTranscript) -- the leaves of ALL the pass's cells in one
// launch of k_sha256_cell_leaves out of the arena, in order on the pass's stream behind the upload, the n x 32 digests down behind an
// event, one ROOT per problem on the host threads while the decoding kernels run.  The roots stay on the host on purpose: a lane per
// problem would serialise n / 2 compressions of a large problem (8192 cells: ~4 k dependent compressions), and the wait for the
// status words is there anyway.  Everything behind the challenge is the same for all four combinations.
// A third source, the COLUMNS of one block over one commitment list (eth_kzg_amd_verify_data_columns / _device; engine.hpp:
// VerifyManyInput::columns): problem b is column b.  The commitments are de-duplicated once per call and decoded once per pass, and
// because all cells of a column carry one index, the second proof product is one per column, h^64 * A_b, behind the reduction of A_b
// (k_verify_many.hip: k_vc_*): n + Bc n_u + Bc scalar multiplications where the expanded pass has 2 n + Bc n_u.  Validation, chunks,
// parts, the short-chain form, the challenges, the fold and the search are the pass's own; the per-column pair is the expanded pass's.
#include "vm_search.hpp"

namespace kzg {

namespace {
using vm::host_threads; using vm::poisoned; using vm::check_pair;  // vm_search.hpp
struct Problem {  // one verification of the call, after validation
    const uint8_t* const* uniq = nullptr;  // de-duplicated commitments, first-occurrence order (verifier.rs:49-65)
    const int* row = nullptr;              // per cell: index into uniq
    std::vector<const uint8_t*> own_uniq;  // where the two live when the problem was de-duplicated alone; the columns of a
    std::vector<int> own_row;              // column call all refer to the call's one pair (verify_host.hpp: ColumnCommitments)
    int n = 0, m = 0;                  // cells, unique commitments (0, 0 when the problem is skipped)
    uint64_t src0 = 0, mir0 = 0;       // (flat device source) its first entry in the caller's arrays / in the pinned mirror
};

// Where a pass's arrays lie: n cells and m unique commitments of Bc problems.  Device arena: [inputs, uploaded in one copy |
// power tables and folding weights, uploaded after the hashes | device only]; the pinned slab holds both uploads and the read-backs.
struct PassLayout {
    const int n, m, Bc;
    const bool small;
    const bool leaf;  // leaf-hashed challenges: n x 32 digest bytes on the device and, read back, in the pinned slab
    // the column source: the m unique commitments are the PASS's (every problem's), each problem has its own m weights, there is no
    // second proof scalar but one h^64 per problem, and the products are n + Bc m, with Bc more slots for the commitment-side sums
    const bool cols;
    const size_t wn = cols ? (size_t)Bc * (size_t)m : (size_t)m;  // (every column of a column pass holds cells: Bc m <= n m / n_blobs <= n)
    const int max_ranges = std::min(Bc, 2048);  // probes per level of the search for wrong proofs
    static constexpr size_t JACQ = launch::SIZEOF_JACQ;
    Carve d;  // (members are initialised in the order they stand here)
    const size_t off_p = d.take((size_t)n * 48), off_c = d.take((size_t)m * 48), off_cells = d.take((size_t)n * BYTES_PER_CELL),
                 off_idx = d.take((size_t)n * 4), off_row = d.take((size_t)n * 4), off_bat = d.take((size_t)n * 4), off_pos = d.take((size_t)n * 4),
                 off_rowb = d.take((size_t)m * 4), off_cs = d.take((size_t)(Bc + 1) * 4), off_rs = d.take((size_t)(Bc + 1) * 4), in_bytes = d.end;
    const size_t off_pow = d.take((size_t)Bc * 24 * sizeof(Fr)),  // second upload (after the hashes)
                 off_rho = d.take((size_t)Bc * 16),               // folding weights, 128 bits per problem
                 in2_bytes = d.end;
    Carve h = d;  // pinned read-backs behind the inputs
    const size_t poff_st = h.take((size_t)(n + m + Bc) * 4), poff_out = h.take((size_t)2 * Bc * JACQ), poff_fold = h.take((size_t)2 * JACQ),
                 poff_rng = h.take((size_t)max_ranges * 8), poff_rsum = h.take((size_t)2 * max_ranges * JACQ), poff_leaf = h.take(leaf ? (size_t)n * 32 : 0),
                 poff_verd = h.take((size_t)max_ranges),  // the verdict bytes of k_pairing_check
                 pin_bytes = h.end;
    // device only
    const size_t off_pts = d.take((size_t)(n + m) * sizeof(G1Affine)), off_evals = d.take((size_t)n * CELL_LEN * sizeof(Fr)),
                 off_coef = d.take((size_t)n * CELL_LEN * sizeof(Fr)),
                 off_stp = d.take((size_t)(n + m) * 4),  // [proofs n | commitments m]
                 off_ste = d.take((size_t)Bc * 4), off_rp = d.take((size_t)n * sizeof(Fr)), off_s1 = d.take((size_t)n * sizeof(Fr)),
                 off_s2 = d.take(cols ? 0 : (size_t)n * sizeof(Fr)), off_h = d.take(cols ? (size_t)Bc * sizeof(Fr) : 0),
                 off_w = d.take(wn * sizeof(Fr)), off_isc = d.take((size_t)Bc * 64 * sizeof(Fr)), off_icm = d.take((size_t)Bc * JACQ),
                 off_prod = d.take(((cols ? (size_t)n + wn + (size_t)Bc : 2 * (size_t)n + (size_t)m) + (small ? 64 * (size_t)Bc : 0)) * JACQ),
                 off_out = d.take((size_t)2 * Bc * JACQ), off_fprod = d.take((size_t)2 * Bc * JACQ), off_fold = d.take((size_t)2 * JACQ),
                 off_rng = d.take((size_t)max_ranges * 8), off_rsum = d.take((size_t)2 * max_ranges * JACQ),
                 off_leaf = d.take(leaf ? (size_t)n * 32 : 0), off_verd = d.take((size_t)max_ranges), dev_bytes = d.end;
    PassLayout(int n_, int m_, int Bc_, bool small_, bool leaf_, bool cols_) : n(n_), m(m_), Bc(Bc_), small(small_), leaf(leaf_), cols(cols_) {}
};

// The host's side of one pass: problems b0 .. b0 + Bc of the call (`in` is the call's input from b0 on), n cells and m unique
// commitments in all, staged into the pinned slab hb as L lays it out.  Nothing in here touches the GPU.
struct PassHost {
    const PassLayout& L;
    const Problem* pr;
    const VerifyManyInput in;
    const uint64_t* mirror_i;  // (flat device source) the pinned mirror of the call's indices: a problem's begin at its mir0
    uint8_t* hb;
    int T;
    HostPool* pool;
    const pairing::G2Prepared* vk[2];        // [tau^64]_2, -[1]_2
    vm::DevicePairing gpu;                   // the same keys for k_pairing_check (the search's larger batches of probes)
    int* verified;                           // verified[i] belongs to problem i of the pass
    std::atomic<int> device_fault{0};
    std::vector<int> cell_start, row_start;  // first cell / first unique commitment of each problem
    std::vector<uint8_t> digests;            // of the challenges: the fold seed hashes them
    std::vector<char> live;                  // problems that decoded without an error
    VerifyManyTap* tap = nullptr;            // (null in the product) receives copies of the read-backs
    const JacQ* sums() const { return (const JacQ*)(hb + L.poff_out); }  // the problems' two sums read back
    int* h_status() const { return (int*)(hb + L.poff_st); }  // read-backs: [proofs n | commitments m | cells, per problem]
    const uint64_t* indices_of(int i) const { return in.on_device() ? mirror_i + pr[i].mir0 : in.cell_indices[i]; }
    uint64_t index_of(int i, int k) const { return in.columns ? in.col_indices[i] : indices_of(i)[k]; }  // of cell k of problem i

    // gather the problems into the slab (flat device source: what the host made of them; proofs and cells move inside HBM); stale
    // contents of the persistent slab must fail closed: status words and result slots are poisoned
    void stage() {
        cell_start.assign(L.Bc + 1, 0); row_start.assign(L.Bc + 1, 0);
        for (int i = 0; i < L.Bc; i++) { cell_start[i + 1] = cell_start[i] + pr[i].n; row_start[i + 1] = L.cols ? 0 : row_start[i] + pr[i].m; }
        if (L.cols)  // the one commitment list of the call, once per pass; rows are pass-wide (row_start is 0 throughout)
            for (int j = 0; j < L.m; j++) memcpy(hb + L.off_c + (size_t)j * 48, in.col->uniq[j], 48);
        memcpy(hb + L.off_cs, cell_start.data(), (size_t)(L.Bc + 1) * 4);
        memcpy(hb + L.off_rs, row_start.data(), (size_t)(L.Bc + 1) * 4);
        int *h_idx = (int*)(hb + L.off_idx), *h_row = (int*)(hb + L.off_row), *h_bat = (int*)(hb + L.off_bat), *h_pos = (int*)(hb + L.off_pos),
            *h_rowb = (int*)(hb + L.off_rowb);
        const bool gather = !in.on_device();
        parallel_for(L.Bc, T, pool, [&](int i) {
            const Problem& p = pr[i];
            const int c0 = cell_start[i], r0 = row_start[i];
            for (int j = 0; j < p.m && !L.cols; j++) { memcpy(hb + L.off_c + (size_t)(r0 + j) * 48, p.uniq[j], 48); h_rowb[r0 + j] = i; }
            for (int k = 0; k < p.n; k++) {
                if (gather) {
                    memcpy(hb + L.off_p + (size_t)(c0 + k) * 48, in.proofs[i][k], 48);
                    memcpy(hb + L.off_cells + (size_t)(c0 + k) * BYTES_PER_CELL, in.cells[i][k], BYTES_PER_CELL);
                }
                h_idx[c0 + k] = (int)index_of(i, k);
                h_row[c0 + k] = r0 + p.row[k];
                h_bat[c0 + k] = i;
                h_pos[c0 + k] = k;
            }
        });
        memset(h_status(), 0xff, (size_t)(L.n + L.m + L.Bc) * 4);
        memset(hb + L.poff_out, 0xff, (size_t)2 * L.Bc * launch::SIZEOF_JACQ);
        memset(hb + L.poff_fold, 0xff, (size_t)2 * launch::SIZEOF_JACQ);
    }
    // the Fiat-Shamir challenges on the host threads, then the table r^(2^i) per problem.  The reference's transcript
    // (verify_host.hpp: CellBatchTranscript) over the caller's buffers, or, for the flat device source, over the proofs and cells that
    // came down into the slab; leaf-hashed: one ROOT per problem over the leaf digests that came down (cell_leaf_root)
    void hash_challenges() {
        Fr* h_pow = (Fr*)(hb + L.off_pow);
        digests.assign((size_t)L.Bc * 32, 0);
        parallel_for(L.Bc, T, pool, [&](int i) {
            const Problem& p = pr[i];
            Fr* tab = h_pow + (size_t)i * 24;
            if (p.n == 0) { for (int j = 0; j < 24; j++) tab[j] = one<FrParams>(); return; }
            Fr cur;
            if (L.leaf) {
                cur = cell_leaf_root(hb + L.poff_leaf, cell_start.data(), (size_t)i, &digests[(size_t)i * 32]);
            } else {
                CellBatchTranscript t(p.m, p.n, p.uniq);
                if (in.on_device()) {
                    const uint8_t *sc = hb + L.off_cells + (size_t)cell_start[i] * BYTES_PER_CELL, *sp = hb + L.off_p + (size_t)cell_start[i] * 48;
                    for (int k = 0; k < p.n; k++) t.absorb(p.row[k], index_of(i, k), sc + (size_t)k * BYTES_PER_CELL, sp + (size_t)k * 48);
                } else {
                    for (int k = 0; k < p.n; k++) t.absorb(p.row[k], index_of(i, k), in.cells[i][k], in.proofs[i][k]);
                }
                cur = t.finish();
                memcpy(&digests[(size_t)i * 32], t.digest(), 32);
            }
            for (int j = 0; j < 24; j++) { tab[j] = cur; cur = sqr(cur); }
        });
    }
    // decoding verdicts per problem (order of the reference: commitments, proofs, cells) -> live problems; the others take no further part
    int judge(int* status) {
        const int* h_st = h_status();
        live.assign(L.Bc, 0);
        int n_live = 0;
        bool shared_bad = false;  // (the column source) a bad commitment of the one list is every column's
        for (int j = 0; j < L.m && L.cols; j++) shared_bad |= h_st[L.n + j] != 0;
        for (int i = 0; i < L.Bc; i++) {
            const Problem& p = pr[i];
            if (p.n == 0) continue;
            const int c0 = cell_start[i], r0 = row_start[i];
            int bad = shared_bad ? (int)ERR_G1 : (int)OK;
            for (int j = 0; j < p.m && !bad && !L.cols; j++) if (h_st[L.n + r0 + j]) bad = ERR_G1;
            for (int k = 0; k < p.n && !bad; k++) if (h_st[c0 + k]) bad = ERR_G1;
            if (!bad && h_st[L.n + L.m + i]) bad = ERR_SCALAR;
            status[i] = bad;
            if (!bad) { live[i] = 1; n_live++; }
        }
        return n_live;
    }
    void check_single(int i) {  // one problem's own pairing check
        const int v = check_pair(sums() + 2 * (size_t)i, vk);
        if (v < 0) device_fault.store(1);
        else verified[i] = v;
    }
    // folding weights (verify_host.hpp: fold_seed, fold_weight); 0 for problems that are out
    void fold_weights() {
        uint32_t* h_rho = (uint32_t*)(hb + L.off_rho);
        uint8_t seed[32];
        fold_seed(digests.data(), digests.size(), seed);
        parallel_for(L.Bc, T, pool, [&](int i) {
            uint32_t* r4 = h_rho + 4 * (size_t)i;
            if (live[i]) fold_weight(seed, (uint64_t)i, r4);
            else r4[0] = r4[1] = r4[2] = r4[3] = 0;
        });
    }
};

// Some proof of the pass is wrong.  The weighted pairs rho_b * sum_b are still in HBM (off_fprod): the search of vm_search.hpp over them;
// where it ends in single problems, each is checked on the host against its own sums, which the pass has read back anyway.
void search_wrong_proofs(PassHost& V, int n_live, uint8_t* db, hipStream_t st) {
    vm::SearchView S = vm::search_view(V.L, V.L.Bc, V.L.off_fprod, V.T, V.pool, V.hb, V.vk, V.gpu, V.live.data(), V.verified, &V.device_fault);
    S.check_single = [&V](int i) { V.check_single(i); };
    if (V.tap) { S.tap_probes = &V.tap->probes; S.tap_probe_sums = &V.tap->probe_sums; S.tap_device_probes = &V.tap->device_probes; }
    vm::search_wrong_proofs(S, n_live, db, st);
    if (V.tap && !V.tap->probes.empty()) V.tap->searched = 1;
}
}  // namespace

int Engine::verify_cell_kzg_proof_batch_many_host(uint64_t n_batches, const uint64_t* n_commitments,
                                                  const uint8_t* const* const* commitments, const uint64_t* n_indices,
                                                  const uint64_t* const* cell_indices, const uint64_t* n_cells,
                                                  const uint8_t* const* const* cells, const uint64_t* n_proofs,
                                                  const uint8_t* const* const* proofs, int* verified, int* status, VerifyManyTap* tap) {
    VerifyManyInput in;
    in.n_commitments = n_commitments; in.n_indices = n_indices; in.n_cells = n_cells; in.n_proofs = n_proofs;
    in.commitments = commitments; in.cell_indices = cell_indices; in.cells = cells; in.proofs = proofs;
    return verify_cell_kzg_proof_batch_many(n_batches, in, verified, status, tap);
}

int Engine::verify_cell_kzg_proof_batch_many(uint64_t n_batches, const VerifyManyInput& in, int* verified, int* status, VerifyManyTap* tap) {
    const int B = (int)n_batches;
    if (in.columns && !in.col_ready) {
        // ---- the column source, once per call: what no column reads anything for; the ONE de-duplication of the call (the device form
        // brings the 48 n_blobs commitment bytes down for it, behind what the caller's stream has queued); and the columns refused at
        // validation taken OUT of the call, so that every column of a pass holds n_blobs cells and the per-(column, commitment) work of
        // a pass (Bc n_u weights and products) is bounded by its cells -- a refused column costs a status word, as in _many
        if (in.col_blobs == 0 || in.col_blobs > MAX_CELLS_PER_VERIFICATION) {
            for (int b = 0; b < B; b++) { status[b] = validate_data_column(in.col_blobs, in.col_indices[b]); verified[b] = status[b] == OK; }
            return OK;
        }
        std::vector<uint64_t> keep;  // the columns that go on, in the caller's order
        for (int b = 0; b < B; b++) {
            verified[b] = 0;
            status[b] = validate_data_column(in.col_blobs, in.col_indices[b]);
            if (status[b] == OK) keep.push_back((uint64_t)b);
        }
        if (keep.empty()) return OK;
        ColumnCommitments cc;
        VerifyManyInput go = in;
        go.col_ready = true;
        if (!in.col) {
            if (in.col_device) {
                try {
                    HIPCK(hipSetDevice(dev_));
                    cc.own.resize((size_t)in.col_blobs * 48);
                    HIPCK(hipStreamSynchronize(in.user_stream));
                    HIPCK(hipMemcpy(cc.own.data(), in.d_commitments, cc.own.size(), hipMemcpyDeviceToHost));
                } catch (const std::exception& e) {
                    set_error(e);
                    return ERR_DEVICE;
                }
                cc.from_own(in.col_blobs);
            } else {
                cc.from_list(in.col_blobs, in.col_commitments);
            }
            go.col = &cc;
        }
        if (keep.size() == (size_t)B) return verify_cell_kzg_proof_batch_many(n_batches, go, verified, status, tap);
        if (tap) return ERR_INPUT;  // (the hook serves calls whose columns all pass validation: its outputs are indexed by column)
        const size_t K = keep.size();
        std::vector<uint64_t> idx(K), src(K);
        std::vector<const uint8_t* const*> cl(in.col_device ? 0 : K), pf(in.col_device ? 0 : K);
        for (size_t k = 0; k < K; k++) {
            idx[k] = in.col_indices[keep[k]];
            src[k] = in.col_src ? in.col_src[keep[k]] : in.col0 + keep[k];
            if (!in.col_device) { cl[k] = in.cells[keep[k]]; pf[k] = in.proofs[keep[k]]; }
        }
        go.col_indices = idx.data();
        if (in.col_device) { go.col_src = src.data(); go.col0 = 0; }
        else { go.cells = cl.data(); go.proofs = pf.data(); }
        std::vector<int> ver(K), st(K);
        const int rc = verify_cell_kzg_proof_batch_many((uint64_t)K, go, ver.data(), st.data(), nullptr);
        if (rc != OK) return rc;
        for (size_t k = 0; k < K; k++) { verified[keep[k]] = ver[k]; status[keep[k]] = st[k]; }
        return OK;
    }
    for (int b = 0; b < B; b++) { verified[b] = 0; status[b] = OK; }
    if (B == 0) return OK;
    // A LARGE call is cut into parts that run as passes of their own on different pass slots at the same time: while one part's
    // products are on the GPU the next one's 100+ MB are still being staged and hashed by the host threads (in one pass the
    // staging of all 275 MB of a 1024-problem call came first, ~10 ms, and the GPU waited for it).  Each part folds its own
    // pairing check (one pass, round 3's form: 28.4-28.9 ms against 24.6-26.2 for 1024 problems).
    constexpr int max_parts = VM_SLOTS < 3 ? (int)VM_SLOTS : 3;
    uint64_t total_cells = 0;
    if (max_parts > 1 && B >= VM_SPLIT_MIN_PROBLEMS)
        for (int b = 0; b < B; b++) total_cells += in.cells_of((uint64_t)b);
    if (total_cells < (uint64_t)VM_SPLIT_MIN_CELLS) return verify_cell_kzg_proof_batch_many_part(B, in, verified, status, tap);
    std::vector<int> cut{0};
    uint64_t acc = 0;
    for (int b = 0; b < B; b++) {  // equal shares of the cells
        acc += in.cells_of((uint64_t)b);
        if ((int)cut.size() < max_parts && acc * max_parts >= total_cells * cut.size() && b + 1 < B) cut.push_back(b + 1);
    }
    cut.push_back(B);
    const int parts = (int)cut.size() - 1;
    std::vector<int> rcs(parts, OK);
    std::vector<std::string> errs(parts);  // (the error text belongs to the thread that ran the part)
    const auto thrown = run_side_by_side(parts, [&](int p) {
        const int lo = cut[p];
        rcs[p] = verify_cell_kzg_proof_batch_many_part(cut[p + 1] - lo, in.from((uint64_t)lo), verified + lo, status + lo, nullptr);
        if (rcs[p] == ERR_DEVICE) errs[p] = last_error();
    });
    for (int p = 0; p < parts; p++) {
        if (thrown[p]) { rcs[p] = ERR_DEVICE; errs[p] = what_was_thrown(thrown[p], "", "unknown failure"); }
        if (rcs[p] != OK) { set_error(std::runtime_error(errs[p])); return rcs[p]; }
    }
    return OK;
}

Engine::VmHost Engine::vm_host() {
    const int T = host_threads(knobs_);
    std::call_once(vm_pool_once_, [&] { vm_pool_.reset(new HostPool(T > 1 ? T - 1 : 1, [d = dev_] { (void)hipSetDevice(d); })); });
    return {T, vm_pool_.get()};
}
vm::DevicePairing Engine::device_pairing(int key) const {
    if (gpu_pairing_min_ <= 0) return {};
    return {d_pairing_key(key), d_pairing_key(1), d_pairing_frob(), gpu_pairing_min_};
}
// A free pass slot (lock, stream, arena, pinned slab); when all are taken, queue on one of them in turn (host_sync.hpp: SlotSet).
// prefer_idle_work_set: first choice is a free slot whose work set (whose in-order stream the pass runs on) is not held by a prover
// call right now -- otherwise the pass and that call wait on each other's work and a fault of either surfaces in both; a
// peek, not a lease: a prover call that takes the set a moment later shares the stream with the pass, which is correct, only serial.
// A slot runs on the stream of one of the prover's three work sets instead of a stream of its own: HIP maps a process's streams onto
// FOUR hardware queues per priority, and the context's stream + the three work-set streams are exactly four -- a fifth stream would
// share a queue with one of them and the two would take turns (seen in the rocprofv3 trace of four concurrent callers).
Engine::PassSlot Engine::lease_pass_slot(bool prefer_idle_work_set) {
    auto work_of = [this](int k) -> Work& { return work_[1 + k % (NW - 1)]; };
    auto lease = prefer_idle_work_set ? vm_slots_.acquire([&](int k) { return mutex_is_free(work_of(k).mu); }) : vm_slots_.acquire();
    const hipStream_t st = work_of(lease.index).stream;
    return {&vm_slot_[lease.index], std::move(lease.lock), st ? st : stream_};
}

int Engine::verify_cell_kzg_proof_batch_many_part(int B, const VerifyManyInput& in, int* verified, int* status, VerifyManyTap* tap) {
    const VmHost host = vm_host();
    const int T = host.T;
    HostPool* const pool = host.pool;
    PassSlot ps = lease_pass_slot(/*prefer_idle_work_set=*/true);
    VmSlot* const slot = ps.slot;
    try {
        HIPCK(hipSetDevice(dev_));
        const hipStream_t st = ps.stream;
        TraceLap lap{knobs_.trace, "verify_many"};
        // ---- flat device source: commitments and indices of the call's cells come down (56 bytes per cell) behind whatever the
        // caller's stream has queued; the host validates and de-duplicates from this pinned mirror, and the unique commitments of a
        // pass are gathered out of it
        // A problem beyond the size bound is refused by its validation below (status 3) and has no place in the mirror: nothing of it is
        // read, and the mirror is sized by problems of at most MAX_CELLS_PER_VERIFICATION cells only.
        const uint8_t* mirror_c = nullptr;
        const uint64_t* mirror_i = nullptr;
        std::vector<Problem> pr(B);
        if (in.columns) {  // (the commitments came down with the call, the indices are the host's: nothing to mirror)
            for (int b = 0; b < B; b++) pr[b].src0 = (in.col_src ? in.col_src[b] : in.col0 + (uint64_t)b) * in.col_blobs;
            if (in.on_device()) order_behind(st, in.user_stream, slot->ordered);
        } else if (in.on_device()) {
            uint64_t N = 0;
            for (int b = 0; b < B; b++) {
                pr[b].src0 = in.cell_starts[b];
                pr[b].mir0 = N;
                if (in.cells_of((uint64_t)b) <= MAX_CELLS_PER_VERIFICATION) N += in.cells_of((uint64_t)b);
            }
            order_behind(st, in.user_stream, slot->ordered);
            if (N) {
                grow_pinned(slot->src_pin, slot->src_pin_cap, (size_t)N * 56);
                uint8_t* const pin_c = slot->src_pin;
                uint64_t* const pin_i = reinterpret_cast<uint64_t*>(slot->src_pin + (size_t)N * 48);
                for (int b = 0; b < B;) {  // one pair of copies per run of problems within the bound (they follow each other in both)
                    uint64_t run = 0;
                    int e = b;
                    while (e < B && in.cells_of((uint64_t)e) <= MAX_CELLS_PER_VERIFICATION) run += in.cells_of((uint64_t)e++);
                    if (run) {
                        HIPCK(hipMemcpyAsync(pin_c + (size_t)pr[b].mir0 * 48, in.d_commitments + (size_t)pr[b].src0 * 48, (size_t)run * 48, hipMemcpyDeviceToHost, st));
                        HIPCK(hipMemcpyAsync(pin_i + pr[b].mir0, in.d_cell_indices + pr[b].src0, (size_t)run * 8, hipMemcpyDeviceToHost, st));
                    }
                    b = e < B ? e + 1 : e;  // (e is the problem beyond the bound that ended the run)
                }
                SYNC_CHECKED(st);
                mirror_c = pin_c;
                mirror_i = pin_i;
            }
            lap("commitments + indices down");
        }
        // ---- per problem: validation (verifier.rs:123-164) and de-duplication
        parallel_for(B, T, pool, [&](int b) {
            const uint64_t nb = in.cells_of((uint64_t)b);
            Problem& p = pr[b];
            if (in.columns) {  // (verify_host.hpp: validate_data_column; every column refers to the call's one de-duplication)
                status[b] = validate_data_column(nb, in.col_indices[b]);
                if (status[b] != OK) return;
                if (nb == 0) { verified[b] = 1; return; }
                p.uniq = in.col->uniq.data(); p.row = in.col->row.data();
                p.n = (int)nb;
                p.m = (int)in.col->uniq.size();
                return;
            }
            if (in.on_device()) {  // (the four lengths are one by construction: what is left is the bound, checked before an index is read, and the indices)
                status[b] = validate_cell_batch(nb, nb, nb, nb, mirror_i + p.mir0);
            } else {
                status[b] = validate_cell_batch(in.n_commitments[b], in.n_indices[b], nb, in.n_proofs[b], in.cell_indices[b]);
            }
            if (status[b] != OK) return;
            if (nb == 0) { verified[b] = 1; return; }  // verifier.rs:90-93
            if (in.on_device()) dedup_commitments_flat(nb, mirror_c + (size_t)p.mir0 * 48, p.own_uniq, p.own_row);
            else dedup_commitments(nb, in.commitments[b], p.own_uniq, p.own_row);
            p.uniq = p.own_uniq.data(); p.row = p.own_row.data();
            p.n = (int)nb;
            p.m = (int)p.own_uniq.size();
        });
        lap("validation + de-duplication");
        // ---- chunks of problems: at most CHUNK_CELLS cells per pass (the pinned slab and the arena stay bounded)
        constexpr int CHUNK_CELLS = VM_CHUNK_CELLS;
        bool fold = true;  // one folded pairing check per pass instead of one per problem (falls back to per-problem checks when it fails)
        if (!knobs_.vm_fold) fold = false;  // (test hook: one pairing per problem)
        for (int b0 = 0; b0 < B;) {
            int b1 = b0, nn = 0, mm = 0;
            while (b1 < B && (b1 == b0 || nn + pr[b1].n <= CHUNK_CELLS)) { nn += pr[b1].n; mm += pr[b1].m; b1++; }
            const int Bc = b1 - b0, n = nn, m = in.columns ? (int)in.col->uniq.size() : mm;  // (columns: the pass's one list)
            if (n == 0) { b0 = b1; continue; }
            // A pass of a few problems (concurrent single calls combined) is a chain of latencies, not work: it takes the SHORT-CHAIN
            // form -- subgroup tests and the interpolation commitments' terms inside the ONE launch of all scalar multiplications
            // (k_vm_products), no fold (its 128-bit multiplication per problem is a 1.4 ms chain; <= 2 T pairing checks are one or
            // two rounds of the host threads) -- decode 0.45 + products 1.7 + sums 0.2 ms of GPU instead of ~6
            const bool small = vm_small_max_ != 0 && Bc <= (vm_small_max_ > 0 ? vm_small_max_ : 2 * T);
            const PassLayout L(n, m, Bc, small, in.leaf, in.columns);
            grow_device(slot->dev, slot->dev_cap, L.dev_bytes, st);
            grow_pinned(slot->pin, slot->pin_cap, L.pin_bytes);
            uint8_t *hb = slot->pin, *db = (uint8_t*)slot->dev;
            PassHost H{L, pr.data() + b0, in.from((uint64_t)b0), mirror_i, hb, T, pool, {g2_tau_.get(), g2_neg_gen_.get()}, device_pairing(0), verified + b0};
            H.tap = tap;
            H.stage();
            lap("stage (host)");
            int* h_st = H.h_status();
            HIPCK(hipMemsetAsync(db + L.off_stp, 0xff, (size_t)(n + m) * 4, st));
            HIPCK(hipMemsetAsync(db + L.off_out, 0xff, (size_t)2 * Bc * launch::SIZEOF_JACQ, st));
            HIPCK(hipMemsetAsync(db + L.off_fold, 0xff, (size_t)2 * launch::SIZEOF_JACQ, st));
            HIPCK(hipMemsetAsync(db + L.off_ste, 0, (size_t)Bc * 4, st));
            if (!in.on_device()) {
                HIPCK(hipMemcpyAsync(db, hb, L.in_bytes, hipMemcpyHostToDevice, st));
            } else {
                // only the host-made parts go up; proofs and cells move inside HBM, from any byte address, one copy per run of
                // problems that follow each other in the caller's arrays (a problem refused at validation leaves a gap)
                HIPCK(hipMemcpyAsync(db + L.off_c, hb + L.off_c, (size_t)m * 48, hipMemcpyHostToDevice, st));
                HIPCK(hipMemcpyAsync(db + L.off_idx, hb + L.off_idx, L.in_bytes - L.off_idx, hipMemcpyHostToDevice, st));
                uint64_t run0 = 0, run = 0, at = 0;
                auto flush = [&] {
                    if (!run) return;
                    HIPCK(hipMemcpyAsync(db + L.off_p + (size_t)at * 48, in.d_proofs + (size_t)run0 * 48, (size_t)run * 48, hipMemcpyDeviceToDevice, st));
                    HIPCK(hipMemcpyAsync(db + L.off_cells + (size_t)at * BYTES_PER_CELL, in.d_cells + (size_t)run0 * BYTES_PER_CELL,
                                         (size_t)run * BYTES_PER_CELL, hipMemcpyDeviceToDevice, st));
                    at += run;
                    run = 0;
                };
                for (int i = 0; i < Bc; i++) {
                    const Problem& p = pr[b0 + i];
                    if (p.n == 0) continue;
                    if (run && p.src0 != run0 + run) flush();
                    if (!run) run0 = p.src0;
                    run += (uint64_t)p.n;
                }
                flush();
                if (!in.leaf) {  // the reference's transcript hashes every byte on the host: the pass's proofs and cells come down, compacted
                    HIPCK(hipMemcpyAsync(hb + L.off_p, db + L.off_p, (size_t)n * 48, hipMemcpyDeviceToHost, st));
                    HIPCK(hipMemcpyAsync(hb + L.off_cells, db + L.off_cells, (size_t)n * BYTES_PER_CELL, hipMemcpyDeviceToHost, st));
                }
            }
            const bool hash_waits = in.leaf || in.on_device();  // the host's hashes read what a copy on st brings down
            if (hash_waits && !slot->hash_inputs_down) HIPCK(hipEventCreateWithFlags(&slot->hash_inputs_down, hipEventDisableTiming));
            if (in.leaf) {
                // the leaves of all the pass's cells straight out of the arena (its offsets are multiples of 256: the kernel's 16-byte
                // loads), in order on the pass's stream: a stream of its own would be a fifth one (lease_pass_slot), and a wave per 64 cells
                // for 35 dependent compressions is short against the decoding behind it
                launch::sha256_cell_leaves(n, db + L.off_c, (const int*)(db + L.off_row), (const int*)(db + L.off_idx), db + L.off_p, db + L.off_cells,
                                           db + L.off_leaf, st, (const int*)(db + L.off_pos));
                HIPCK(hipMemcpyAsync(hb + L.poff_leaf, db + L.off_leaf, (size_t)n * 32, hipMemcpyDeviceToHost, st));
            }
            if (hash_waits) HIPCK(hipEventRecord(slot->hash_inputs_down, st));
            // ---- challenge-free GPU work: decode (on curve) + subgroup tests of [proofs | commitments], cells, interpolation
            G1Affine* d_pts = (G1Affine*)(db + L.off_pts);
            int* d_stp = (int*)(db + L.off_stp);
            launch::g1_decode2(db + L.off_p, d_pts, d_stp, n, db + L.off_c, d_pts + n, d_stp + n, m, beta_, st);
            if (!small) launch::g1_subgroup2(d_pts, d_stp, n, d_pts + n, d_stp + n, m, beta_, st);  // (small: inside k_vm_products)
            launch::cells_to_fr(db + L.off_cells, db + L.off_evals, nullptr, (int*)(db + L.off_ste), (const int*)(db + L.off_bat), nullptr, n, st);
            launch::interp_cells(db + L.off_evals, (const int*)(db + L.off_idx), d_w8192_, inv64_, db + L.off_coef, n, st);
            HIPCK(hipMemcpyAsync(h_st, d_stp, (size_t)(n + m) * 4, hipMemcpyDeviceToHost, st));
            HIPCK(hipMemcpyAsync(h_st + n + m, db + L.off_ste, (size_t)Bc * 4, hipMemcpyDeviceToHost, st));
            HIPCK(hipGetLastError());
            lap("enqueue (host)");
            if (hash_waits) HIPCK(hipEventSynchronize(slot->hash_inputs_down));
            H.hash_challenges();  // meanwhile, on the host threads
            lap(in.leaf ? "leaf hashes (GPU) + roots (host)" : "sha256 transcripts (host)");
            SYNC_CHECKED(st);     // (the challenge-free GPU work has long finished under the hashes: a short wait)
            lap("wait decode");
            int n_live = H.judge(status + b0);  // (a small pass judges again once its subgroup tests are in)
            const bool folded = fold && n_live >= 2 && !small;
            if (folded) H.fold_weights();
            HIPCK(hipMemcpyAsync(db + L.off_pow, hb + L.off_pow, L.in2_bytes - L.off_pow, hipMemcpyHostToDevice, st));  // power tables + weights
            // ---- per-problem scalars, weights, interpolation sums; every scalar multiplication; the two sums per problem
            const int *d_cs = (const int*)(db + L.off_cs), *d_rs = (const int*)(db + L.off_rs);
            // one sequence for both sources (launch.hpp: a null pointer tells a launcher which).  The column source has r^k per cell and ONE
            // h^64 per column: n + Bc m products over the one decoded commitment table, then h^64 A_b as a dependent launch of Bc quads
            // behind the reduction of A_b, inside vm_sums
            const bool cols = in.columns;
            launch::vm_scalars(db + L.off_pow, (const int*)(db + L.off_bat), (const int*)(db + L.off_pos), (const int*)(db + L.off_idx), d_cs, d_w8192_,
                               db + L.off_rp, db + L.off_s1, cols ? nullptr : db + L.off_s2, cols ? db + L.off_h : nullptr, n, Bc, st);
            launch::vm_weights(db + L.off_rp, (const int*)(db + L.off_row), cols ? nullptr : (const int*)(db + L.off_rowb), d_cs, db + L.off_w, m, Bc, st);
            launch::vm_interp_sum(db + L.off_coef, db + L.off_rp, d_cs, db + L.off_isc, Bc, st);
            uint64_t muls = (uint64_t)launch::vm_products(d_pts, db + L.off_s1, cols ? nullptr : db + L.off_s2, db + L.off_w, db + L.off_isc, d_srs_,
                                                          db + L.off_prod, n, m, Bc, small, d_stp, beta_, st);
            // - commit(interpolation polynomial): 64 fixed bases = group 0 of the commitment window table (verification_key.rs:66-70)
            if (!small) launch_msm(db + L.off_isc, TAB_SRS, db + L.off_icm, 1, Bc, Bc, 0, st, launch::FMT_JACQ);
            muls += (uint64_t)launch::vm_sums(db + L.off_prod, small ? nullptr : db + L.off_icm, d_cs, cols ? nullptr : d_rs, db + L.off_h, db + L.off_out,
                                              n, m, Bc, beta_, st);
            if (small) HIPCK(hipMemcpyAsync(h_st, d_stp, (size_t)(n + m) * 4, hipMemcpyDeviceToHost, st));  // with the subgroup verdicts now
            if (folded) {
                launch::vm_fold(db + L.off_out, (const uint32_t*)(db + L.off_rho), db + L.off_fprod, db + L.off_fold, Bc, beta_, st);
                HIPCK(hipMemcpyAsync(hb + L.poff_fold, db + L.off_fold, (size_t)2 * launch::SIZEOF_JACQ, hipMemcpyDeviceToHost, st));
            }
            HIPCK(hipMemcpyAsync(hb + L.poff_out, db + L.off_out, (size_t)2 * Bc * launch::SIZEOF_JACQ, hipMemcpyDeviceToHost, st));
            SYNC_CHECKED(st);
            lap("scalars + products + sums (GPU)");
            if (small) n_live = H.judge(status + b0);
            if (tap) {
                tap->digests = H.digests;
                if (in.leaf) tap->leaves.assign(hb + L.poff_leaf, hb + L.poff_leaf + (size_t)n * 32);
                tap->passes++;
                tap->small = small; tap->folded = folded;
                tap->commitments_decoded = (uint64_t)m; tap->scalar_muls = muls;
                tap->sums.assign(hb + L.poff_out, hb + L.poff_out + (size_t)2 * Bc * launch::SIZEOF_JACQ);
                tap->rho.assign((const uint32_t*)(hb + L.off_rho), (const uint32_t*)(hb + L.off_rho) + 4 * (size_t)Bc);
                if (folded) tap->fold.assign(hb + L.poff_fold, hb + L.poff_fold + (size_t)2 * launch::SIZEOF_JACQ);
            }
            // ---- verdicts: ONE pairing check of the folded sums; only if that fails (some problem's proof is wrong) one per problem
            bool all_true = false;
            if (folded) {
                const int v = check_pair((const JacQ*)(hb + L.poff_fold), H.vk);
                if (v < 0) throw std::runtime_error("many-verification pass left no folded result");
                all_true = v == 1;
                if (tap) tap->fold_verdict = v;
            }
            if (all_true) {
                for (int i = 0; i < Bc; i++)
                    if (H.live[i]) {
                        if (poisoned(H.sums()[2 * (size_t)i]) || poisoned(H.sums()[2 * (size_t)i + 1])) { H.device_fault.store(1); break; }
                        verified[b0 + i] = 1;
                    }
            } else if (folded && vm_search_) {
                search_wrong_proofs(H, n_live, db, st);
            } else {
                parallel_for(Bc, T, pool, [&](int i) {
                    if (H.live[i]) H.check_single(i);
                });
            }
            if (H.device_fault.load()) throw std::runtime_error("many-verification pass left no result");
            lap("pairing checks (host)");
            b0 = b1;
        }
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// ---------------------------------------------------------------------------------------------------------------
struct Engine::VerifyRequest {
    uint64_t n[4];
    const uint8_t* const* commitments;
    const uint64_t* cell_indices;
    const uint8_t* const* cells;
    const uint8_t* const* proofs;
    int verified = 0, status = OK;
    bool done = false;
    bool taken = false;  // a leader has this request in its pass (its owner then only waits)
    std::string error;  // of a device failure of the pass that carried this request
};

int Engine::verify_cell_kzg_proof_batch_combined(uint64_t n_commitments, const uint8_t* const* commitments, uint64_t n_indices,
                                                 const uint64_t* cell_indices, uint64_t n_cells, const uint8_t* const* cells,
                                                 uint64_t n_proofs, const uint8_t* const* proofs, int* verified) {
    *verified = 0;
    const bool enabled = knobs_.verify_combine;
    // ONE caller at a time (verify_lanes_), a large batch, or the feature switched off: the latency-optimised single path (3.3 ms);
    // callers that arrive while it is taken are combined into passes on the three pass slots (a pass of 1-8 problems: 3.7-4.1 ms
    // in the short-chain form).  Round 3 sent the first four callers to four engine lanes; their streams shared hardware queues
    // with each other (HIP has four per process), and lanes cannot share launches the way a pass does: measured this round,
    // verifications/s at 2 / 4 / 8 / 16 / 32 threads: four lanes 450 / 650 / 906 / 1997 / 3703, one lane 523 / 681 / 1284 / 2291 / 4323
    if (!enabled || n_cells > (uint64_t)comb_max_cells_ || verify_inflight_.fetch_add(1) < verify_lanes_) {
        struct Leave { std::atomic<int>* c; bool on; ~Leave() { if (on) c->fetch_sub(1); } } leave{&verify_inflight_, enabled && n_cells <= (uint64_t)comb_max_cells_};
        auto lane = lease_serial();
        const int st = lane.e->verify_cell_kzg_proof_batch_host(n_commitments, commitments, n_indices, cell_indices, n_cells, cells, n_proofs,
                                                                proofs, verified);
        if (st == ERR_DEVICE && lane.e != this) set_error(std::runtime_error(lane.e->last_error()));
        return st;
    }
    verify_inflight_.fetch_sub(1);  // this call goes through the combiner instead
    VerifyRequest me;
    me.n[0] = n_commitments; me.n[1] = n_indices; me.n[2] = n_cells; me.n[3] = n_proofs;
    me.commitments = commitments; me.cell_indices = cell_indices; me.cells = cells; me.proofs = proofs;
    // leader election, follower wake-up and the release of the followers whatever happens in a pass: host_sync.hpp (Combiner), which
    // tests/c/test_host_sync.cpp drives under ThreadSanitizer with fake passes
    combiner_.submit(me, [&](std::vector<VerifyRequest*>& batch) {
    const size_t B = batch.size();
    // whatever happens in here (an allocation failure included) the followers must be released with a verdict: a leader that
    // left with comb_running_ set would leave every queued and every later caller waiting for ever
    int rc = ERR_DEVICE;
    std::string why;
    std::vector<int> ver, st;
    try {
      if (B == 1) {
        // a "pass" of one problem is the single path itself -- 3.3 ms against the 3.65 of a one-problem pass (its points are
        // shifted before the challenge; a pass multiplies by per-lane scalars after it) -- on a pass slot's stream and arena:
        // the latency lane and three slots make four single verifications side by side, one hardware queue each
        PassSlot sl = lease_pass_slot(/*prefer_idle_work_set=*/false);
        VmSlot* slot = sl.slot;
        slot->vs.stream = sl.stream;
        VerifyRequest* r = batch[0];
        G1Affine pts[2];
        bool empty = false;
        ver.assign(1, 0);
        st.assign(1, (int)ERR_DEVICE);
        HIPCK(hipSetDevice(dev_));
        st[0] = verify_cells_partial(r->n[0], r->commitments, r->n[1], r->cell_indices, r->n[2], r->cells, r->n[3], r->proofs, 0, r->n[2], pts, &empty, nullptr, &slot->vs);
        sl.lock.unlock();  // the pairing needs no slot
        rc = st[0] == ERR_DEVICE ? (int)ERR_DEVICE : (int)OK;
        if (rc == ERR_DEVICE) why = last_error();
        if (st[0] == OK) ver[0] = (empty || verify_cells_pairing_split(pts)) ? 1 : 0;
      } else {
        std::vector<uint64_t> l0(B), l1(B), l2(B), l3(B);
        std::vector<const uint8_t* const*> pc(B), pl(B), pp(B);
        std::vector<const uint64_t*> pi(B);
        ver.assign(B, 0);
        st.assign(B, (int)ERR_DEVICE);
        for (size_t i = 0; i < B; i++) {
            l0[i] = batch[i]->n[0]; l1[i] = batch[i]->n[1]; l2[i] = batch[i]->n[2]; l3[i] = batch[i]->n[3];
            pc[i] = batch[i]->commitments; pi[i] = batch[i]->cell_indices; pl[i] = batch[i]->cells; pp[i] = batch[i]->proofs;
        }
        rc = verify_cell_kzg_proof_batch_many_host(B, l0.data(), pc.data(), l1.data(), pi.data(), l2.data(), pl.data(), l3.data(),
                                                   pp.data(), ver.data(), st.data());
        if (rc == ERR_DEVICE) why = last_error();
      }
    } catch (const std::exception& e) {
        rc = ERR_DEVICE;
        why = std::string("combined verification pass: ") + e.what();
    } catch (...) {
        rc = ERR_DEVICE;
        why = "combined verification pass: unknown failure";
    }
        for (size_t i = 0; i < B; i++) {
            batch[i]->status = (rc == ERR_DEVICE || i >= st.size()) ? (int)ERR_DEVICE : st[i];
            batch[i]->verified = i < ver.size() ? ver[i] : 0;
            batch[i]->error = why;
        }
    }, [&](std::vector<VerifyRequest*>& batch, const std::string& what) {
        for (VerifyRequest* r : batch) { r->status = ERR_DEVICE; r->verified = 0; r->error = "combined verification pass: " + what; }
    });
    if (me.status == ERR_DEVICE) set_error(std::runtime_error(me.error));  // the error text belongs to the calling thread
    *verified = me.status == OK ? me.verified : 0;
    return me.status;
}

}  // namespace kzg
