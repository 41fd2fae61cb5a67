// eth_kzg_amd_verify_cell_kzg_proof_batch_many: MANY independent verify_cell_kzg_proof_batch problems in one call.
// Reference semantics per problem: DASContext::verify_cell_kzg_proof_batch (crates/eip7594/src/verifier.rs:72-164) ->
// FK20Verifier::verify_multi_opening (crates/cryptography/kzg_multi_open/src/fk20/verifier.rs:129-260); the reference gets
// its throughput by verifying from many threads on one context (bindings/node/src/lib.rs:92-299,
// crates/cryptography/bls12_381/src/lib.rs:45-50).  Here the problems of a call share every GPU launch.
// FOUR SOURCES (engine.hpp: VerifyManyInput says what each holds), resolved once per part into a CellSource: pointer lists on the
// host; flat arrays in HBM plus cell_starts; the columns of one block over ONE commitment list, on the host or in HBM (problem b is
// column b; verify_data_columns_many does the source's once-per-call work; its PARTIAL spelling: a column holds the blobs of its bitmap
// only, and its weights and products go by a sparse (column, commitment) pair list); blobs with their commitment and 128 cell proofs, on the host
// or in HBM (problem b is blob b's 128 cells, which the pass computes itself in its arena: the step `extend`).  Two challenges: the reference's transcript per problem,
// or the leaf-hashed challenge of each problem alone (verify_host.hpp: CellLeafTranscript).  A large CALL is cut into at most three
// concurrent PARTS, a part into CHUNKS of at most VM_CHUNK_CELLS cells, and every chunk is one PASS (Engine::CellManyPass) on one of three
// pass slots (lease_pass_slot); the plans are verify_host.hpp's.  Nothing here takes the context's big lock.  The steps of a pass:
//   arena      the slot's blocks, large enough; the result slots of the slab poisoned
//   stage      host threads: the problems into the pinned slab (host sources: proofs and cells; all: commitments, indices, rows)
//   upload     ONE copy up; device sources: the host-made arrays up, proofs and cells device-to-device in copy runs (and down
//              again, compacted, for the reference's transcript); the blob source: only the blob halves of the cells
//   extend     (the blob source) cells 64..127 of every blob into the second half of its slice, in place (k_ntt.hip: k_blob_to_extension)
//   leaves     (leaf-hashed) the leaves of ALL the pass's cells in one launch of k_sha256_cell_leaves out of the arena, n x 32 bytes down
//   decode     decode + subgroup-check all points, decode all cells, per-cell interpolation: challenge-free, behind the hashes
//   challenges host threads: one SHA-256 transcript, or one ROOT over the leaf digests, per problem (on the host on purpose: a lane per problem
//              would serialise n / 2 compressions, and the wait for the status words is there anyway); the decoding verdicts; the folding weights
//   products_and_sums   scalars / weights / interpolation sums, ONE LANE PER SCALAR MULTIPLICATION (k_verify_many.hip), the 64-term
//              interpolation commitments from the commitment window table, the two sums per problem (small passes: the short chain)
//   fold_and_sums_down  the problems' sums folded on the GPU with 127-bit weights derived from all the challenges; both down
//   verdicts   ONE 2-pairing check per pass; where it fails the wrong problems are SEARCHED by folding sub-ranges of the resident weighted sums,
//              one pairing per probe ($ETH_KZG_AMD_VM_SEARCH=0: one by one; $ETH_KZG_AMD_VM_FOLD=0: no fold)
#include "vm_search.hpp"
#include <memory>
#include <numeric>

namespace kzg {

namespace {
using vm::host_threads; using vm::poisoned; using vm::check_pair;  // vm_search.hpp
struct Problem {  // one verification of the call, after validation
    const uint8_t* const* uniq = nullptr;  // de-duplicated commitments, first-occurrence order (verifier.rs:49-65)
    const int* row = nullptr;              // per cell: index into uniq
    std::vector<const uint8_t*> own_uniq;  // where the two live when the problem was de-duplicated alone; the columns of a
    std::vector<int> own_row;              // column call all refer to the call's one pair (verify_host.hpp: ColumnCommitments)
    int n = 0, m = 0;                  // cells, unique commitments (0, 0 when the problem is skipped)
    // (partial columns, verify_host.hpp: PartialColumnView) uniq / row / m above are the TRANSCRIPT's view, the column's own list and the
    // rows re-ranked inside it; the kernels read the pass-wide row of every cell, and the column's pairs are its list in pass-wide rows
    std::unique_ptr<PartialColumnView> pv;  // (null for every other source: they pay a pointer)
    const int* pass_row = nullptr;     // per cell: the row the kernels read (null: row)
    int pairs() const { return pv ? (int)pv->pair_u.size() : 0; }
};

// Where the B problems of a part come from: made once per part, it answers what the part and its passes ask about problem b.
struct CellSource {
    const VerifyManyInput in;  // the part's input
    const int B;
    const bool device = in.on_device();  // proofs and cells lie in HBM (the host has neither)
    const bool shared = in.columns;      // the commitments are the pass's: one list, every problem's (the column source)
    const bool partial = in.part != nullptr;  // (the column source) a bitmap of blobs per column: unequal columns, a pair list per pass
    const bool blobs = in.from_blobs;    // a problem is a blob: its cells are computed in the arena, its indices are 0..127, one commitment
    std::vector<uint64_t> src0;          // (device) the problem's first entry in the caller's d_cells / d_proofs
    std::vector<uint64_t> mir0;          // (flat arrays) its first entry in the pinned mirror of commitments and indices: back to back
    uint64_t mirror_n = 0;               // entries of the mirror
    const uint8_t* mirror_c = nullptr;   // set by mirror_down
    const uint64_t* mirror_i = nullptr;
    CellSource(const VerifyManyInput& in_, int B_) : in(in_), B(B_) {
        for (int b = 0; b < B && device; b++) {
            src0.push_back(blobs ? (uint64_t)b * N_CELLS : partial ? in.part->start[part_at(b)] : shared ? place(b) * in.col_blobs : in.cell_starts[b]);
            mir0.push_back(mirror_n);
            if (!shared && !blobs && in_mirror(b)) mirror_n += cells_of(b);
        }
    }
    uint64_t cells_of(int b) const { return in.cells_of((uint64_t)b); }
    // a problem beyond the size bound is refused by its validation (status 3) and has no place in the mirror: nothing of it is read
    bool in_mirror(int b) const { return cells_of(b) <= MAX_CELLS_PER_VERIFICATION; }
    uint64_t place(int b) const { return shared ? in.col_place[b] : (uint64_t)b; }  // where the caller's arrays hold problem b
    uint64_t part_at(int b) const { return in.part_base + place(b); }               // (partial columns) its column in the call's PartialColumns
    uint64_t index_of(int b, int k) const {
        return blobs ? (uint64_t)k : shared ? in.col_indices[place(b)] : device ? mirror_i[mir0[b] + k] : in.cell_indices[b][k];
    }
    const uint8_t* cell(int b, int k) const { return in.cells[place(b)][k]; }  // (host sources)
    const uint8_t* blob(int b) const { return in.blobs[b]; }                   // (the blob source on the host)
    // (the blob source) the problem's one commitment: the caller's bytes, or what commitments_down brought
    const uint8_t* blob_commitment(int b) const { return device ? mirror_c + (size_t)b * 48 : in.blob_commitments[b]; }
    const uint8_t* proof(int b, int k) const { return in.proofs[place(b)][k]; }
    int pass_m() const { return shared ? (int)in.col->uniq.size() : 0; }  // the pass-wide commitments
    const uint8_t* const* pass_uniq() const { return shared ? in.col->uniq.data() : nullptr; }
    int own_rows(const Problem& p) const { return shared ? 0 : p.m; }     // the commitments a problem brings into a pass itself
    // validation (verifier.rs:123-164; flat arrays: the bound, checked before an index is read, and the indices) and de-duplication
    // of problem b -> its status; p is filled only if the problem goes on
    int admit(int b, Problem& p) const {
        const uint64_t nb = cells_of(b);
        if (blobs) {  // lengths and indices hold by construction (verify_host.hpp): nothing to validate, one commitment, every row 0
            static const int row0[N_CELLS] = {};
            p.own_uniq.assign(1, blob_commitment(b));
            p.uniq = p.own_uniq.data(); p.row = row0;
            p.m = 1; p.n = N_CELLS;
            return OK;
        }
        if (partial) {  // validated with the call (only accepted columns come here); the column's own list, rows and pairs
            if (nb == 0) return OK;
            p.pv.reset(new PartialColumnView);
            partial_column_view(*in.col, in.part->blob.data() + in.part->blob_start[part_at(b)], nb, *p.pv);
            p.uniq = p.pv->uniq.data(); p.row = p.pv->row.data(); p.pass_row = p.pv->pass_row.data();
            p.m = (int)p.pv->uniq.size(); p.n = (int)nb;
            return OK;
        }
        const int st = shared   ? validate_data_column(nb, in.col_indices[place(b)])
                       : device ? validate_cell_batch(nb, nb, nb, nb, mirror_i + mir0[b])
                                : validate_cell_batch(in.n_commitments[b], in.n_indices[b], nb, in.n_proofs[b], in.cell_indices[b]);
        if (st != OK || nb == 0) return st;
        if (shared) {  // every column refers to the call's one de-duplication
            p.uniq = in.col->uniq.data(); p.row = in.col->row.data();
            p.m = (int)in.col->uniq.size();
        } else {
            if (device) dedup_commitments_flat(nb, mirror_c + (size_t)mir0[b] * 48, p.own_uniq, p.own_row);
            else dedup_commitments(nb, in.commitments[b], p.own_uniq, p.own_row);
            p.uniq = p.own_uniq.data(); p.row = p.own_row.data();
            p.m = (int)p.own_uniq.size();
        }
        p.n = (int)nb;
        return st;
    }
};
// flat arrays: commitments and indices of the part's cells come down (56 bytes per cell) into the pinned mirror (pin, cap: the
// slot's), one pair of copies per run of problems within the bound
void mirror_down(CellSource& S, uint8_t*& pin, size_t& cap, hipStream_t st) {
    if (!S.mirror_n) return;
    grow_pinned(pin, cap, (size_t)S.mirror_n * 56);
    uint64_t* const pin_i = reinterpret_cast<uint64_t*>(pin + (size_t)S.mirror_n * 48);
    for (const CopyRun& r : vm_copy_runs(S.B, [&](int b) { return S.src0[b]; }, [&](int b) { return S.cells_of(b); }, [&](int b) { return S.in_mirror(b); })) {
        HIPCK(hipMemcpyAsync(pin + (size_t)r.dst * 48, S.in.d_commitments + (size_t)r.src * 48, (size_t)r.len * 48, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(pin_i + r.dst, S.in.d_cell_indices + r.src, (size_t)r.len * 8, hipMemcpyDeviceToHost, st));
    }
    SYNC_CHECKED(st);
    S.mirror_c = pin; S.mirror_i = pin_i;
}
// the blob source in HBM: the part's B x 48 commitment bytes come down for the passes' commitment rows (nothing else of the source does)
void commitments_down(CellSource& S, uint8_t*& pin, size_t& cap, hipStream_t st) {
    grow_pinned(pin, cap, (size_t)S.B * 48);
    HIPCK(hipMemcpyAsync(pin, S.in.d_commitments, (size_t)S.B * 48, hipMemcpyDeviceToHost, st));
    SYNC_CHECKED(st);
    S.mirror_c = pin;
}

// Where a pass's arrays lie: n cells and m unique commitments of Bc problems.  Device arena: [inputs, uploaded in one copy |
// power tables and folding weights, uploaded after the hashes | device only]; the pinned slab holds both uploads and the read-backs.
struct PassLayout {
    const int n, m, Bc;
    const bool small;
    const bool leaf;  // leaf-hashed challenges: n x 32 digest bytes on the device and, read back, in the pinned slab
    // the column source: the m unique commitments are the PASS's (every problem's), each problem has its own m weights, there is no
    // second proof scalar but one h^64 per problem, and the products are n + Bc m, with Bc more slots for the commitment-side sums
    const bool cols;
    // partial columns: P (column, commitment) pairs in place of Bc m, P <= n always since every pair has a cell (-1: no pair list)
    const int P;
    const size_t wn = P >= 0 ? (size_t)P : cols ? (size_t)Bc * (size_t)m : (size_t)m;  // (every column of a dense pass holds cells: Bc m <= n m / n_blobs <= n)
    const int max_ranges = std::min(Bc, 2048);  // probes per level of the search for wrong proofs
    static constexpr size_t JACQ = launch::SIZEOF_JACQ;
    Carve d;  // (members are initialised in the order they stand here)
    const size_t off_p = d.take((size_t)n * 48), off_c = d.take((size_t)m * 48), off_cells = d.take((size_t)n * BYTES_PER_CELL),
                 off_idx = d.take((size_t)n * 4), off_row = d.take((size_t)n * 4), off_bat = d.take((size_t)n * 4), off_pos = d.take((size_t)n * 4),
                 off_rowb = d.take((size_t)m * 4), off_cs = d.take((size_t)(Bc + 1) * 4), off_rs = d.take((size_t)(Bc + 1) * 4),
                 off_ps = d.take(P >= 0 ? (size_t)(Bc + 1) * 4 : 0), off_pu = d.take(P >= 0 ? (size_t)P * 4 : 0),  // pair_start, pair_u
                 in_bytes = d.end;
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
    PassLayout(int n_, int m_, int Bc_, bool small_, bool leaf_, bool cols_, int P_)
        : n(n_), m(m_), Bc(Bc_), small(small_), leaf(leaf_), cols(cols_), P(P_) {}
};
}  // namespace

// One pass: problems [b0, b0 + Bc) of a part (pr: the first of them; problem i is the source's b0 + i) on the part's slot and its stream
// st, its steps in the order run() takes them; the tap (null in the product) receives copies of the read-backs in the step that has them.
struct Engine::CellManyPass {
    Engine& e;
    const CellSource& S;
    const Problem* const pr;
    const int b0, Bc;
    int *const ver, *const stat;  // the pass's verdicts and statuses in the caller's arrays
    VerifyManyTap* const tap;
    const int T;
    HostPool* const pool;
    VmSlot* const slot;
    const hipStream_t st;
    TraceLap& lap;
    static int cells(const Problem* pr, int Bc) { return std::accumulate(pr, pr + Bc, 0, [](int a, const Problem& p) { return a + p.n; }); }
    const int n = cells(pr, Bc);
    const int m = S.shared ? S.pass_m() : std::accumulate(pr, pr + Bc, 0, [](int a, const Problem& p) { return a + p.m; });  // unique commitments
    // A pass of a few problems (concurrent single calls combined) is a chain of latencies, not work: it takes the SHORT-CHAIN form --
    // subgroup tests and the interpolation commitments' terms inside the ONE launch of all scalar multiplications (k_vm_products), no fold
    // (a 1.4 ms chain; <= 2 T pairing checks are one or two rounds of the host threads) -- 0.45 + 1.7 + 0.2 ms of GPU instead of ~6
    const bool small = e.vm_small_max_ != 0 && Bc <= (e.vm_small_max_ > 0 ? e.vm_small_max_ : 2 * T);
    const int P = S.partial ? std::accumulate(pr, pr + Bc, 0, [](int a, const Problem& p) { return a + p.pairs(); }) : -1;  // the pass's pairs
    const PassLayout L{n, m, Bc, small, S.in.leaf, S.shared, P};
    const pairing::G2Prepared* const vk[2] = {e.g2_tau_.get(), e.g2_neg_gen_.get()};  // [tau^64]_2, -[1]_2
    const vm::DevicePairing gpu = e.device_pairing(0);  // the same keys for k_pairing_check (the search's larger batches of probes)
    // the host's hashes read what a copy on st brings down: the leaf digests, or the proofs and cells of a device source
    const bool hash_waits = L.leaf || S.device;
    uint8_t *hb = nullptr, *db = nullptr;    // the slot's pinned slab and device arena
    std::atomic<int> device_fault{0};
    std::vector<int> cell_start, row_start;  // first cell / first unique commitment of each problem
    std::vector<int> pair_start;             // (partial columns) first pair of each column
    std::vector<uint8_t> digests;            // of the challenges: the fold seed hashes them
    std::vector<char> live;                  // problems that decoded without an error
    int n_live = 0;
    bool folded = false;  // one folded pairing check for the pass instead of one per problem
    const JacQ* sums() const { return (const JacQ*)(hb + L.poff_out); }  // the problems' two sums read back
    int* h_status() const { return (int*)(hb + L.poff_st); }  // read-backs: [proofs n | commitments m | cells, per problem]

    void run() {
        arena();
        stage();
        upload();
        extend();
        columns();
        leaves();
        decode();
        challenges();
        products_and_sums();
        fold_and_sums_down();
        verdicts();
        columns_out();
    }
    // the slot's blocks, large enough; stale contents of the persistent slab must fail closed: status words and result slots are poisoned
    void arena() {
        grow_device(slot->dev, slot->dev_cap, L.dev_bytes, st);
        grow_pinned(slot->pin, slot->pin_cap, L.pin_bytes);
        hb = slot->pin, db = (uint8_t*)slot->dev;
        memset(h_status(), 0xff, (size_t)(L.n + L.m + L.Bc) * 4);
        memset(hb + L.poff_out, 0xff, (size_t)2 * L.Bc * launch::SIZEOF_JACQ);
        memset(hb + L.poff_fold, 0xff, (size_t)2 * launch::SIZEOF_JACQ);
        if (tap) { tap->passes++; tap->small = small; tap->commitments_decoded = (uint64_t)m; }
    }
    // ---- gather the problems into the slab (device sources: what the host made of them); the commitments: every problem's own
    // behind each other, or the pass's one list (rows are then pass-wide: row_start is 0 throughout)
    void stage() {
        cell_start.assign(Bc + 1, 0); row_start.assign(Bc + 1, 0);
        for (int i = 0; i < Bc; i++) { cell_start[i + 1] = cell_start[i] + pr[i].n; row_start[i + 1] = row_start[i] + S.own_rows(pr[i]); }
        for (int j = 0; j < S.pass_m(); j++) memcpy(hb + L.off_c + (size_t)j * 48, S.pass_uniq()[j], 48);
        memcpy(hb + L.off_cs, cell_start.data(), (size_t)(Bc + 1) * 4);
        memcpy(hb + L.off_rs, row_start.data(), (size_t)(Bc + 1) * 4);
        if (S.partial) {  // the pair list: column i's pairs are its own unique list, as indices into the pass's commitments
            pair_start.assign(Bc + 1, 0);
            for (int i = 0; i < Bc; i++) pair_start[i + 1] = pair_start[i] + pr[i].pairs();
            memcpy(hb + L.off_ps, pair_start.data(), (size_t)(Bc + 1) * 4);
            int* const h_pu = (int*)(hb + L.off_pu);
            for (int i = 0; i < Bc; i++) if (pr[i].pv) std::copy(pr[i].pv->pair_u.begin(), pr[i].pv->pair_u.end(), h_pu + pair_start[i]);
        }
        int *h_idx = (int*)(hb + L.off_idx), *h_row = (int*)(hb + L.off_row), *h_bat = (int*)(hb + L.off_bat), *h_pos = (int*)(hb + L.off_pos),
            *h_rowb = (int*)(hb + L.off_rowb);
        const bool gather = !S.device;
        parallel_for(Bc, T, pool, [&](int i) {
            const Problem& p = pr[i];
            const int c0 = cell_start[i], r0 = row_start[i];
            for (int j = 0; j < S.own_rows(p); j++) { memcpy(hb + L.off_c + (size_t)(r0 + j) * 48, p.uniq[j], 48); h_rowb[r0 + j] = i; }
            if (gather && S.blobs) memcpy(hb + L.off_cells + blob_cells_slice((size_t)i).blob_at, S.blob(b0 + i), BYTES_PER_BLOB);  // cells 0..63
            for (int k = 0; k < p.n; k++) {
                if (gather) {
                    memcpy(hb + L.off_p + (size_t)(c0 + k) * 48, S.proof(b0 + i, k), 48);
                    if (!S.blobs) memcpy(hb + L.off_cells + (size_t)(c0 + k) * BYTES_PER_CELL, S.cell(b0 + i, k), BYTES_PER_CELL);
                }
                h_idx[c0 + k] = (int)S.index_of(b0 + i, k);
                h_row[c0 + k] = p.pass_row ? p.pass_row[k] : r0 + p.row[k];
                h_bat[c0 + k] = i;
                h_pos[c0 + k] = k;
            }
        });
        lap("stage (host)");
    }
    // ---- the device's result slots poisoned, then the inputs into the arena
    void upload() {
        HIPCK(hipMemsetAsync(db + L.off_stp, 0xff, (size_t)(n + m) * 4, st));
        HIPCK(hipMemsetAsync(db + L.off_out, 0xff, (size_t)2 * Bc * launch::SIZEOF_JACQ, st));
        HIPCK(hipMemsetAsync(db + L.off_fold, 0xff, (size_t)2 * launch::SIZEOF_JACQ, st));
        HIPCK(hipMemsetAsync(db + L.off_ste, 0, (size_t)Bc * 4, st));
        constexpr size_t slice = 2 * (size_t)BYTES_PER_BLOB;  // (the blob source) a blob's 128 cells; its first half is the blob
        if (!S.device && S.blobs) {  // the empty halves stay where they are: [proofs, commitments], the blob halves (one strided copy), the rest
            HIPCK(hipMemcpyAsync(db, hb, L.off_cells, hipMemcpyHostToDevice, st));
            HIPCK(hipMemcpy2DAsync(db + L.off_cells, slice, hb + L.off_cells, slice, BYTES_PER_BLOB, (size_t)Bc, hipMemcpyHostToDevice, st));
            HIPCK(hipMemcpyAsync(db + L.off_idx, hb + L.off_idx, L.in_bytes - L.off_idx, hipMemcpyHostToDevice, st));
            return;
        }
        if (!S.device) {
            HIPCK(hipMemcpyAsync(db, hb, L.in_bytes, hipMemcpyHostToDevice, st));
            return;
        }
        // only the host-made parts go up; proofs and cells move inside HBM, from any byte address, one copy per run of problems
        // that follow each other in the caller's arrays (a problem refused at validation leaves a gap)
        HIPCK(hipMemcpyAsync(db + L.off_c, hb + L.off_c, (size_t)m * 48, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(db + L.off_idx, hb + L.off_idx, L.in_bytes - L.off_idx, hipMemcpyHostToDevice, st));
        for (const CopyRun& r : vm_copy_runs(Bc, [&](int i) { return S.src0[b0 + i]; }, [&](int i) { return pr[i].n; }, [&](int i) { return pr[i].n != 0; })) {
            HIPCK(hipMemcpyAsync(db + L.off_p + (size_t)r.dst * 48, S.in.d_proofs + (size_t)r.src * 48, (size_t)r.len * 48, hipMemcpyDeviceToDevice, st));
            if (S.blobs) {  // the run's blobs (128 entries each) into the first halves of their slices: one strided copy
                HIPCK(hipMemcpy2DAsync(db + L.off_cells + (size_t)r.dst * BYTES_PER_CELL, slice, S.in.d_blobs + (size_t)(r.src / N_CELLS) * BYTES_PER_BLOB,
                                       BYTES_PER_BLOB, BYTES_PER_BLOB, (size_t)(r.len / N_CELLS), hipMemcpyDeviceToDevice, st));
                continue;
            }
            HIPCK(hipMemcpyAsync(db + L.off_cells + (size_t)r.dst * BYTES_PER_CELL, S.in.d_cells + (size_t)r.src * BYTES_PER_CELL,
                                 (size_t)r.len * BYTES_PER_CELL, hipMemcpyDeviceToDevice, st));
        }
        if (!L.leaf) {  // the reference's transcript hashes every byte on the host: the pass's proofs and cells come down, compacted
            HIPCK(hipMemcpyAsync(hb + L.off_p, db + L.off_p, (size_t)n * 48, hipMemcpyDeviceToHost, st));
            HIPCK(hipMemcpyAsync(hb + L.off_cells, db + L.off_cells, (size_t)n * BYTES_PER_CELL, hipMemcpyDeviceToHost, st));
        }
    }
    // ---- (the blob source) every blob's cells 64..127 behind its bytes; a refused blob sets its problem's cell-status word (which upload
    // has zeroed on this stream) and gets zeros, so that the leaves and the decoding read nothing stale
    void extend() {
        if (S.blobs) launch::blob_to_extension(Bc, db + L.off_cells, (int*)(db + L.off_ste), e.d_w29_, e.n_inv4096_, st);
    }
    // ---- (the blob source of a call that also builds the block's data columns: S.in.out, eth_kzg_amd_blobs_to_data_columns under its flag)
    // The arena holds every item's 128 cells blob-major, which the leaves and the decoding need as they are; the column matrix is a COPY of
    // them behind the extension step (a copy kernel, not a second destination of k_blob_to_extension, whose launch stays
    // what it was), and the proofs are re-ordered from where the pass holds them.  Device source: both into the caller's matrices, for
    // every item of the pass (the slots of an item that fails are unspecified).  Host source: only the extension halves come down, into the
    // halves of the pinned slab's slices that the staging left empty; columns_out hands them over once the verdicts are in.
    void columns() {
        const VerifyManyInput::BlobColumnsOut& o = S.in.out;
        if (!S.blobs) return;
        const launch::Columns cols{(size_t)o.n_total, (size_t)o.first + (size_t)b0};
        if (o.d_cells) launch::cells_to_columns(Bc, db + L.off_cells, o.d_cells, cols, st);
        if (o.d_proofs) launch::proofs_to_columns(Bc, db + L.off_p, o.d_proofs, cols, st);
        constexpr size_t slice = 2 * (size_t)BYTES_PER_BLOB;
        if (o.cells)
            HIPCK(hipMemcpy2DAsync(hb + L.off_cells + blob_cells_slice(0).ext_at, slice, db + L.off_cells + blob_cells_slice(0).ext_at, slice, BYTES_PER_BLOB,
                                   (size_t)Bc, hipMemcpyDeviceToHost, st));
    }
    // ---- (the same, host source) behind the verdicts: the slots of the items that PASSED, and of no other.  Cells 0..63 and the proofs are
    // the caller's own bytes, copied on the host; cells 64..127 are what columns() brought down (fold_and_sums_down has synchronised)
    void columns_out() {
        const VerifyManyInput::BlobColumnsOut& o = S.in.out;
        if (!S.blobs || S.device || (!o.cells && !o.proofs)) return;
        parallel_for(Bc, T, pool, [&](int i) {
            if (!ver[i] || stat[i] != OK) return;
            const size_t at = (size_t)o.first + (size_t)b0 + (size_t)i;
            const uint8_t *const blob = S.blob(b0 + i), *const ext = hb + L.off_cells + blob_cells_slice((size_t)i).ext_at;
            for (int c = 0; c < N_CELLS && o.cells; c++)
                memcpy(o.cells[c][at], c < N_CELLS / 2 ? blob + (size_t)c * BYTES_PER_CELL : ext + (size_t)(c - N_CELLS / 2) * BYTES_PER_CELL, BYTES_PER_CELL);
            for (int c = 0; c < N_CELLS && o.proofs; c++) memcpy(o.proofs[c][at], S.proof(b0 + i, c), 48);
        });
        lap("columns out (host)");
    }
    // ---- (leaf-hashed) the leaves of all the pass's cells straight out of the arena (its offsets are multiples of 256: the kernel's
    // 16-byte loads), in order on the pass's stream (a fifth stream: lease_pass_slot).  The event: what the host threads hash is down.
    void leaves() {
        if (hash_waits && !slot->hash_inputs_down) HIPCK(hipEventCreateWithFlags(&slot->hash_inputs_down, hipEventDisableTiming));
        if (L.leaf) {
            launch::sha256_cell_leaves(n, db + L.off_c, (const int*)(db + L.off_row), (const int*)(db + L.off_idx), db + L.off_p, db + L.off_cells,
                                       db + L.off_leaf, st, (const int*)(db + L.off_pos));
            HIPCK(hipMemcpyAsync(hb + L.poff_leaf, db + L.off_leaf, (size_t)n * 32, hipMemcpyDeviceToHost, st));
        }
        if (hash_waits) HIPCK(hipEventRecord(slot->hash_inputs_down, st));
    }
    // ---- challenge-free GPU work: decode (on curve) + subgroup tests of [proofs | commitments], cells, interpolation
    void decode() {
        G1Affine* d_pts = (G1Affine*)(db + L.off_pts);
        int* d_stp = (int*)(db + L.off_stp);
        launch::g1_decode2(db + L.off_p, d_pts, d_stp, n, db + L.off_c, d_pts + n, d_stp + n, m, e.beta_, st);
        if (!small) launch::g1_subgroup2(d_pts, d_stp, n, d_pts + n, d_stp + n, m, e.beta_, st);  // (small: inside k_vm_products)
        launch::cells_to_fr(db + L.off_cells, db + L.off_evals, nullptr, (int*)(db + L.off_ste), (const int*)(db + L.off_bat), nullptr, n, st);
        launch::interp_cells(db + L.off_evals, (const int*)(db + L.off_idx), e.d_w8192_, e.inv64_, db + L.off_coef, n, st);
        HIPCK(hipMemcpyAsync(h_status(), d_stp, (size_t)(n + m) * 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(h_status() + n + m, db + L.off_ste, (size_t)Bc * 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipGetLastError());
        lap("enqueue (host)");
    }
    // ---- meanwhile, on the host threads: the challenges; then the decoding verdicts, the live problems and their folding weights
    void challenges() {
        if (hash_waits) HIPCK(hipEventSynchronize(slot->hash_inputs_down));
        hash_challenges();
        lap(L.leaf ? "leaf hashes (GPU) + roots (host)" : "sha256 transcripts (host)");
        SYNC_CHECKED(st);  // (the challenge-free GPU work has long finished under the hashes: a short wait)
        lap("wait decode");
        n_live = judge();  // (a small pass judges again once its subgroup tests are in)
        folded = e.knobs_.vm_fold && n_live >= 2 && !small;  // (the knob is a test hook: one pairing per problem)
        if (folded) fold_weights();
        if (tap) {
            tap->digests = digests;
            if (L.leaf) tap->leaves.assign(hb + L.poff_leaf, hb + L.poff_leaf + (size_t)n * 32);
            tap->folded = folded;
        }
    }
    // the Fiat-Shamir challenges, then the table r^(2^i) per problem: the reference's transcript (verify_host.hpp: CellBatchTranscript) over
    // the caller's buffers or what a device source brought down into the slab, or one ROOT over the leaf digests (cell_leaf_root)
    void hash_challenges() {
        Fr* h_pow = (Fr*)(hb + L.off_pow);
        digests.assign((size_t)Bc * 32, 0);
        const bool slab = S.device;
        parallel_for(Bc, T, pool, [&](int i) {
            const Problem& p = pr[i];
            Fr* tab = h_pow + (size_t)i * 24;
            if (p.n == 0) { for (int j = 0; j < 24; j++) tab[j] = one<FrParams>(); return; }
            Fr cur;
            if (L.leaf) {
                cur = cell_leaf_root(hb + L.poff_leaf, cell_start.data(), (size_t)i, &digests[(size_t)i * 32]);
            } else {
                CellBatchTranscript t(p.m, p.n, p.uniq);
                const uint8_t *sc = hb + L.off_cells + (size_t)cell_start[i] * BYTES_PER_CELL, *sp = hb + L.off_p + (size_t)cell_start[i] * 48;
                for (int k = 0; k < p.n; k++) {
                    const uint8_t* const cell = slab ? sc + (size_t)k * BYTES_PER_CELL : S.cell(b0 + i, k);
                    const uint8_t* const proof = slab ? sp + (size_t)k * 48 : S.proof(b0 + i, k);
                    t.absorb(p.row[k], S.index_of(b0 + i, k), cell, proof);
                }
                cur = t.finish();
                memcpy(&digests[(size_t)i * 32], t.digest(), 32);
            }
            for (int j = 0; j < 24; j++) { tab[j] = cur; cur = sqr(cur); }
        });
    }
    // decoding verdicts per problem (order of the reference: commitments, proofs, cells; the blob source: the blob first, verify_host.hpp:
    // blob_cells_item_status) -> live problems; the others take no further part
    int judge() {
        const int* h_st = h_status();
        live.assign(Bc, 0);
        int alive = 0;
        bool shared_bad = false;  // a bad commitment of the pass's one list is every problem's; partial columns: of the columns that hold it
        for (int j = 0; j < S.pass_m() && !S.partial; j++) shared_bad |= h_st[L.n + j] != 0;
        for (int i = 0; i < Bc; i++) {
            const Problem& p = pr[i];
            if (p.n == 0) continue;
            const int c0 = cell_start[i], r0 = row_start[i];
            int bad = shared_bad ? (int)ERR_G1 : (int)OK;
            for (int j = 0; j < S.own_rows(p) && !bad; j++) if (h_st[L.n + r0 + j]) bad = ERR_G1;
            for (int j = 0; j < p.pairs() && !bad; j++) if (h_st[L.n + p.pv->pair_u[j]]) bad = ERR_G1;
            for (int k = 0; k < p.n && !bad; k++) if (h_st[c0 + k]) bad = ERR_G1;
            if (!bad && h_st[L.n + L.m + i]) bad = ERR_SCALAR;
            if (S.blobs) bad = blob_cells_item_status(h_st[L.n + L.m + i] != 0, bad == ERR_G1);
            stat[i] = bad;
            if (!bad) { live[i] = 1; alive++; }
        }
        return alive;
    }
    // folding weights (verify_host.hpp: fold_seed, fold_weight); 0 for problems that are out
    void fold_weights() {
        uint32_t* h_rho = (uint32_t*)(hb + L.off_rho);
        uint8_t seed[32];
        fold_seed(digests.data(), digests.size(), seed);
        parallel_for(Bc, T, pool, [&](int i) {
            uint32_t* r4 = h_rho + 4 * (size_t)i;
            if (live[i]) fold_weight(seed, (uint64_t)i, r4);
            else r4[0] = r4[1] = r4[2] = r4[3] = 0;
        });
    }
    // ---- per-problem scalars, weights, interpolation sums; every scalar multiplication; the two sums per problem.  Where the column
    // source's kernels differ a null pointer tells the launcher (launch.hpp), each stated once here: r^k per cell and ONE h^64 per column,
    // weights per (column, commitment), n + Bc m products, and h^64 A_b as a dependent launch behind the reduction of A_b, inside vm_sums
    void products_and_sums() {
        HIPCK(hipMemcpyAsync(db + L.off_pow, hb + L.off_pow, L.in2_bytes - L.off_pow, hipMemcpyHostToDevice, st));  // power tables + weights
        const int* const d_cs = (const int*)(db + L.off_cs);
        int* const d_stp = (int*)(db + L.off_stp);
        uint8_t *const d_s2 = L.cols ? nullptr : db + L.off_s2, *const d_h = L.cols ? db + L.off_h : nullptr;  // vm_scalars, vm_products
        const int* const d_rowb = L.cols ? nullptr : (const int*)(db + L.off_rowb);                                // vm_weights
        const int* const d_rs = L.cols ? nullptr : (const int*)(db + L.off_rs);                                    // vm_sums
        // (partial columns) the pair list: weights, the w C products and the commitment-side sums go by it
        const launch::VmPairs pairs = {S.partial ? (const int*)(db + L.off_ps) : nullptr, S.partial ? (const int*)(db + L.off_pu) : nullptr, S.partial ? P : 0};
        launch::vm_scalars(db + L.off_pow, (const int*)(db + L.off_bat), (const int*)(db + L.off_pos), (const int*)(db + L.off_idx), d_cs, e.d_w8192_,
                           db + L.off_rp, db + L.off_s1, d_s2, d_h, n, Bc, st);
        launch::vm_weights(db + L.off_rp, (const int*)(db + L.off_row), d_rowb, d_cs, db + L.off_w, m, Bc, st, pairs);
        launch::vm_interp_sum(db + L.off_coef, db + L.off_rp, d_cs, db + L.off_isc, Bc, st);
        uint64_t muls = (uint64_t)launch::vm_products(db + L.off_pts, db + L.off_s1, d_s2, db + L.off_w, db + L.off_isc, e.d_srs_, db + L.off_prod, n, m, Bc,
                                                      small, d_stp, e.beta_, st, pairs);
        // - commit(interpolation polynomial): 64 fixed bases = group 0 of the commitment window table (verification_key.rs:66-70)
        if (!small) e.launch_msm(db + L.off_isc, TAB_SRS, db + L.off_icm, 1, Bc, Bc, 0, st, launch::FMT_JACQ);
        muls += (uint64_t)launch::vm_sums(db + L.off_prod, small ? nullptr : db + L.off_icm, d_cs, d_rs, db + L.off_h, db + L.off_out, n, m, Bc, e.beta_, st, pairs);
        if (small) HIPCK(hipMemcpyAsync(h_status(), d_stp, (size_t)(n + m) * 4, hipMemcpyDeviceToHost, st));  // with the subgroup verdicts now
        if (tap) tap->scalar_muls = muls;
    }
    // ---- the fold of a folded pass, then both results down
    void fold_and_sums_down() {
        if (folded) {
            launch::vm_fold(db + L.off_out, (const uint32_t*)(db + L.off_rho), db + L.off_fprod, db + L.off_fold, Bc, e.beta_, st);
            HIPCK(hipMemcpyAsync(hb + L.poff_fold, db + L.off_fold, (size_t)2 * launch::SIZEOF_JACQ, hipMemcpyDeviceToHost, st));
        }
        HIPCK(hipMemcpyAsync(hb + L.poff_out, db + L.off_out, (size_t)2 * Bc * launch::SIZEOF_JACQ, hipMemcpyDeviceToHost, st));
        SYNC_CHECKED(st);
        lap("scalars + products + sums (GPU)");
        if (small) n_live = judge();
        if (tap) {
            tap->sums.assign(hb + L.poff_out, hb + L.poff_out + (size_t)2 * Bc * launch::SIZEOF_JACQ);
            tap->rho.assign((const uint32_t*)(hb + L.off_rho), (const uint32_t*)(hb + L.off_rho) + 4 * (size_t)Bc);
            if (folded) tap->fold.assign(hb + L.poff_fold, hb + L.poff_fold + (size_t)2 * launch::SIZEOF_JACQ);
        }
    }
    // ---- verdicts: ONE pairing check of the folded sums; only if that fails (some problem's proof is wrong) one per problem
    void verdicts() {
        bool all_true = false;
        if (folded) {
            const int v = check_pair((const JacQ*)(hb + L.poff_fold), vk);
            if (v < 0) throw std::runtime_error("many-verification pass left no folded result");
            all_true = v == 1;
            if (tap) tap->fold_verdict = v;
        }
        if (all_true) {
            for (int i = 0; i < Bc; i++)
                if (live[i]) {
                    if (poisoned(sums()[2 * (size_t)i]) || poisoned(sums()[2 * (size_t)i + 1])) { device_fault.store(1); break; }
                    ver[i] = 1;
                }
        } else if (folded && e.vm_search_) {
            search_wrong_proofs();
        } else {
            parallel_for(Bc, T, pool, [&](int i) { if (live[i]) check_single(i); });
        }
        if (device_fault.load()) throw std::runtime_error("many-verification pass left no result");
        lap("pairing checks (host)");
    }
    void check_single(int i) {  // one problem's own pairing check
        const int v = check_pair(sums() + 2 * (size_t)i, vk);
        if (v < 0) device_fault.store(1);
        else ver[i] = v;
    }
    // Some proof of the pass is wrong.  The weighted pairs rho_b * sum_b are still in HBM (off_fprod): the search of vm_search.hpp over
    // them; where it ends in single problems, each is checked on the host against its own sums, which the pass has read back anyway.
    void search_wrong_proofs() {
        vm::SearchView V = vm::search_view(L, Bc, L.off_fprod, T, pool, hb, vk, gpu, live.data(), ver, &device_fault);
        V.check_single = [this](int i) { check_single(i); };
        if (tap) { V.tap_probes = &tap->probes; V.tap_probe_sums = &tap->probe_sums; V.tap_device_probes = &tap->device_probes; }
        vm::search_wrong_proofs(V, n_live, db, st);
        if (tap && !tap->probes.empty()) tap->searched = 1;
    }
};

VerifyManyInput VerifyManyInput::host_partial_columns(const PartialColumns& part, const uint8_t* const* commitments, const uint64_t* column_indices,
                                                      const uint8_t* const* const* cells, const uint8_t* const* const* proofs, bool leaf) {
    VerifyManyInput in = host_columns(part.n_blobs, commitments, column_indices, cells, proofs, leaf);
    in.part = &part; in.part_count = part.count.data();
    return in;
}
VerifyManyInput VerifyManyInput::device_partial_columns(const PartialColumns& part, const uint8_t* d_commitments, const uint64_t* column_indices,
                                                        const uint8_t* d_cells, const uint8_t* d_proofs, hipStream_t user_stream, bool leaf) {
    VerifyManyInput in = device_columns(part.n_blobs, d_commitments, column_indices, d_cells, d_proofs, user_stream, leaf);
    in.part = &part; in.part_count = part.count.data();
    return in;
}

int Engine::verify_cell_kzg_proof_batch_many(uint64_t n_batches, const VerifyManyInput& in, int* verified, int* status, VerifyManyTap* tap) {
    return in.columns ? verify_data_columns_many((int)n_batches, in, verified, status, tap)
                      : verify_cell_kzg_proof_batch_many_parts((int)n_batches, in, verified, status, tap);
}

// The column source, once per call: the ONE de-duplication (the device form brings the 48 n_blobs commitment bytes down for it, behind
// what the caller's stream has queued; a host-form call sliced over a device list brings in.col, made once for all slices); and the
// columns refused at validation taken OUT, so that every column of a pass holds n_blobs cells and its Bc n_u weights and products are
// bounded by its cells.  keep[k]: the caller's column that goes on as problem k (in.col_place); the verdicts are scattered back by it.
// Partial columns (in.part: validated and counted by the caller, once): the kept columns hold m_b cells each, a column without a bit is
// an empty problem, and a call whose kept columns hold no cell reads nothing.
int Engine::verify_data_columns_many(int B, const VerifyManyInput& in, int* verified, int* status, VerifyManyTap* tap) {
    const std::vector<uint64_t> keep = in.part ? vm_kept_partial_columns(*in.part, in.part_base, (uint64_t)B) : vm_kept_columns(in.col_blobs, (uint64_t)B, in.col_indices);
    const size_t K = keep.size();
    for (int b = 0; b < B; b++) { verified[b] = in.col_blobs == 0; status[b] = ERR_INPUT; }  // (no blobs: empty problems, verifier.rs:90-93)
    for (size_t k = 0; k < K; k++) status[keep[k]] = OK;
    uint64_t kept_cells = in.part ? 0 : (uint64_t)K * in.col_blobs;
    for (size_t k = 0; k < K && in.part; k++) {  // (partial columns: a column without a bit is an empty problem)
        const uint64_t m_k = in.part->count[in.part_base + keep[k]];
        verified[keep[k]] = m_k == 0;
        kept_cells += m_k;
    }
    if (kept_cells == 0) return OK;  // (nothing to read: neither the commitments nor a cell)
    ColumnCommitments cc;
    VerifyManyInput go = in;
    if (!in.col && in.col_device) {
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
    } else if (!in.col) {
        cc.from_list(in.col_blobs, in.col_commitments);
    }
    if (!in.col) go.col = &cc;
    go.col_place = keep.data();
    if (K == (size_t)B) return verify_cell_kzg_proof_batch_many_parts(B, go, verified, status, tap);
    if (tap) return ERR_INPUT;  // (the hook serves calls whose columns all pass validation: its outputs are indexed by column)
    std::vector<int> ver(K), st(K);
    const int rc = verify_cell_kzg_proof_batch_many_parts((int)K, go, ver.data(), st.data(), nullptr);
    if (rc != OK) return rc;
    for (size_t k = 0; k < K; k++) { verified[keep[k]] = ver[k]; status[keep[k]] = st[k]; }
    return OK;
}

// The body every source shares.  A LARGE call is cut into parts that run as passes of their own on different pass slots at the same
// time: while one part's products are on the GPU the next one's 100+ MB are still being staged and hashed by the host threads (in one
// pass the staging of a 1024-problem call came first, ~10 ms, and the GPU waited: 28.4-28.9 ms against 24.6-26.2).  Each part folds alone.
int Engine::verify_cell_kzg_proof_batch_many_parts(int B, const VerifyManyInput& in, int* verified, int* status, VerifyManyTap* tap) {
    for (int b = 0; b < B; b++) { verified[b] = 0; status[b] = OK; }
    if (B == 0) return OK;
    constexpr int max_parts = VM_SLOTS < 3 ? (int)VM_SLOTS : 3;
    const std::vector<int> cut = vm_call_parts(B, [&](int b) { return in.cells_of((uint64_t)b); }, VM_SPLIT_MIN_PROBLEMS, VM_SPLIT_MIN_CELLS, max_parts);
    const int parts = (int)cut.size() - 1;
    if (parts == 1) return verify_cell_kzg_proof_batch_many_part(B, in, verified, status, tap);
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

// One part: the slot, the source (flat arrays: the mirror down), validation and de-duplication per problem, then a pass per chunk of
// at most VM_CHUNK_CELLS cells that holds a cell (the pinned slab and the arena stay bounded)
int Engine::verify_cell_kzg_proof_batch_many_part(int B, const VerifyManyInput& in, int* verified, int* status, VerifyManyTap* tap) {
    const VmHost host = vm_host();
    PassSlot ps = lease_pass_slot(/*prefer_idle_work_set=*/true);
    try {
        HIPCK(hipSetDevice(dev_));
        TraceLap lap{knobs_.trace, "verify_many"};
        CellSource S(in, B);
        if (S.device) order_behind(ps.stream, in.user_stream, ps.slot->ordered);
        if (S.device && S.blobs) {
            commitments_down(S, ps.slot->src_pin, ps.slot->src_pin_cap, ps.stream);
            lap("commitments down");
        } else if (S.device && !S.shared) {  // (columns: the commitments came down with the call, the indices are the host's: nothing to mirror)
            mirror_down(S, ps.slot->src_pin, ps.slot->src_pin_cap, ps.stream);
            lap("commitments + indices down");
        }
        std::vector<Problem> pr(B);
        parallel_for(B, host.T, host.pool, [&](int b) {
            status[b] = S.admit(b, pr[b]);
            if (status[b] == OK && pr[b].n == 0) verified[b] = 1;  // verifier.rs:90-93
        });
        lap("validation + de-duplication");
        for (int b0 = 0, b1 = 0; b0 < B; b0 = b1) {
            b1 = vm_chunk_end(B, b0, [&](int b) { return (uint64_t)pr[b].n; }, (uint64_t)VM_CHUNK_CELLS);
            if (CellManyPass::cells(pr.data() + b0, b1 - b0) == 0) continue;
            CellManyPass{*this, S, pr.data() + b0, b0, b1 - b0, verified + b0, status + b0, tap, host.T, host.pool, ps.slot, ps.stream, lap}.run();
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
        rc = verify_cell_kzg_proof_batch_many(B, VerifyManyInput::lists(l0.data(), pc.data(), l1.data(), pi.data(), l2.data(), pl.data(), l3.data(), pp.data(),
                                                                        /*leaf=*/false), ver.data(), st.data());
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
