// Host-side mirror of the reference's DASContext for the GPU hot path
// (reference: crates/eip7594/src/lib.rs:41-87 DASContext, prover.rs:62-171 ProverContext,
//  verifier.rs:72-112).  One Engine = one context on one GPU.
#pragma once
#include "knobs.hpp"
#include "host_sync.hpp"
#include "trusted_setup.hpp"
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <string>
#include <utility>
#include <vector>
#include <memory>

namespace kzg {

namespace pairing { struct G2Prepared; }
namespace vm { struct DevicePairing; }  // vm_search.hpp
struct Comm;  // multi_gpu.cpp
struct ColumnCommitments;  // verify_host.hpp
struct PartialColumns;
struct G1Affine;  // curve.hpp
namespace launch { struct Columns; }  // launch.hpp: the [column][blob] output layout
struct Fr8 { uint32_t v[8]; };
struct Fp12w { uint32_t v[12]; };

// A verification problem's cell list is bounded: the powers of the Fiat-Shamir challenge come from a 24-entry table r^(2^i)
// (k_verify.hip: k_verify_scalars, k_verify_many.hip: k_vm_scalars) and positions are 32-bit on the device.  2^24 cells are 34 GB
// of input; longer lists are rejected as invalid input by every verification entry point.
constexpr uint64_t MAX_CELLS_PER_VERIFICATION = (1u << 24) - 1;
// How verify_cell_kzg_proof_batch_many divides a call (verify_many.hip; the plans themselves: verify_host.hpp): a call of at least VM_SPLIT_MIN_PROBLEMS problems and
// VM_SPLIT_MIN_CELLS cells is cut into concurrent parts, and a pass holds at most VM_CHUNK_CELLS cells (1024 verifications of 128
// cells: 275 MB of pinned staging, ~1 GB of device arena)
constexpr int VM_SPLIT_MIN_PROBLEMS = 192, VM_SPLIT_MIN_CELLS = 24576, VM_CHUNK_CELLS = 131072;
// Tap of a many-verification pass (null in every product call; the stage hook test_verify_many_sums sets it): copies of what the pass's
// pinned read-backs held after the syncs the pass makes anyway, in the kernels' own words (JacQ = launch::SIZEOF_JACQ bytes).
struct VerifyManyTap {
    int passes = 0;                                  // passes the call ran (the hook serves calls of one pass)
    int small = 0, folded = 0, searched = 0;         // the form of the pass
    int fold_verdict = -1;                           // of the folded check (folded passes)
    std::vector<uint8_t> sums;                       // [Bc][2] JacQ: the problems' two sums
    std::vector<uint32_t> rho;                       // [Bc][4]: the folding weights as uploaded
    std::vector<uint8_t> fold;                       // [2] JacQ: the folded pair
    std::vector<int> probes;                         // the search's probes in order: lo, hi, passed
    std::vector<uint8_t> probe_sums;                 // [probe][2] JacQ
    int device_probes = 0;                           // probes whose pairing ran on the GPU (k_pairing_check); the others ran on the host threads
    std::vector<uint8_t> digests;                    // [Bc][32]: the digest each problem's challenge was reduced from (zero: not hashed)
    std::vector<uint8_t> leaves;                     // (leaf-hashed challenges) [n][32]: the leaf digests of the pass's cells as they came down
    uint64_t commitments_decoded = 0;                // commitment points handed to the pass's decoding launches (a launch argument, not a device counter)
    uint64_t scalar_muls = 0;                        // 255-bit products of decoded points its launchers were given (proofs, commitments, h^64 A_b)
};
// Where the problems of a many-verification call come from (verify_many.hip), and how they take their challenges.
//   pointer lists (cell_starts null): problem b has n_*[b] entries in commitments[b] / cell_indices[b] / cells[b] / proofs[b], all on the host
//   flat arrays in this GPU's HBM (cell_starts set, on the host, n_batches + 1 non-decreasing entries): problem b is the entries
//     [cell_starts[b], cell_starts[b + 1]) of d_commitments (48 B each, one per cell), d_cell_indices, d_cells (2048 B), d_proofs (48 B);
//     what user_stream has queued produces them
//   a column matrix over ONE commitment list (columns set; eth_kzg_amd_verify_data_columns / _device): problem b is column b, col_blobs
//     cells that all carry the index col_indices[b] (host) and whose commitments are the call's, one per cell: col_commitments[i],
//     cells[b][i], proofs[b][i] on the host, or (col_device) d_commitments 48 col_blobs bytes, d_cells / d_proofs [columns][col_blobs]
//     entries in this GPU's HBM.  Once the call has taken its refused columns out (verify_many.hip), problem b is the caller's column
//     col_place[b] in all of these.  col: the commitments de-duplicated once for the whole call (null: the call makes it)
//     Partial columns (part set; eth_kzg_amd_verify_partial_data_columns / _device): column b holds cells and proofs for the blobs of its
//     bitmap only, part->count[b] of them, and in HBM the columns lie packed from entry part->start[b] on.
//   blobs with their 128 cell proofs (from_blobs; eth_kzg_amd_verify_blob_cell_proofs_many / _many_device): problem b is the blob's 128
//     cells with the indices 0..127 under ONE commitment; the pass computes the cells itself (k_ntt.hip: k_blob_to_extension) and the
//     challenge is always the leaf-hashed one.  blobs[b] -> 131072 bytes, blob_commitments[b] -> 48 bytes, proofs[b][k] -> 48 bytes on the
//     host, or (blobs_device) d_blobs n x 131072 bytes (4-byte aligned), d_commitments n x 48, d_proofs n x 128 x 48 in this GPU's HBM
// leaf: every problem's challenge is the leaf-hashed one of the problem alone (verify_host.hpp: CellLeafTranscript, cell_leaf_root),
// the leaves hashed on the GPU out of the pass's arena; else the reference's transcript on the host threads.
struct VerifyManyInput {
    const uint64_t *n_commitments = nullptr, *n_indices = nullptr, *n_cells = nullptr, *n_proofs = nullptr, *cell_starts = nullptr;
    const uint8_t *const *const *commitments = nullptr, *const *const *cells = nullptr, *const *const *proofs = nullptr;
    const uint64_t* const* cell_indices = nullptr;
    const uint8_t *d_commitments = nullptr, *d_cells = nullptr, *d_proofs = nullptr;
    const uint64_t* d_cell_indices = nullptr;
    hipStream_t user_stream = nullptr;
    bool leaf = false, columns = false, col_device = false;
    uint64_t col_blobs = 0;
    const uint64_t *col_place = nullptr, *col_indices = nullptr;
    const uint8_t* const* col_commitments = nullptr;
    const PartialColumns* part = nullptr;  // (partial columns) the call's columns; problem b is its column part_base + (col_place ? col_place[b] : b)
    const uint64_t* part_count = nullptr;  // part->count: m of every column of the call
    uint64_t part_base = 0;
    const ColumnCommitments* col = nullptr;
    bool from_blobs = false, blobs_device = false;
    const uint8_t *const *blobs = nullptr, *const *blob_commitments = nullptr;
    const uint8_t* d_blobs = nullptr;
    // (the blob source; eth_kzg_amd_blobs_to_data_columns under its flag) the call also BUILDS the block's data columns from what the pass
    // holds anyway: item i's 128 cells and its 128 proofs as the caller gave them, at [c][first + i] of the WHOLE call's arrays of n_total
    // blobs -- pointer tables on the host (written for the items that pass, behind the verdicts) or matrices in this GPU's HBM
    // ([128][n_total][2048], 4-byte aligned, and [128][n_total][48]: written for every item of a pass, behind its extension step).
    // Each may be null.
    struct BlobColumnsOut {
        uint8_t *const *const *cells = nullptr, *const *const *proofs = nullptr;
        uint8_t *d_cells = nullptr, *d_proofs = nullptr;
        uint64_t n_total = 0, first = 0;
    } out;
    static VerifyManyInput lists(const uint64_t* n_commitments, const uint8_t* const* const* commitments, const uint64_t* n_indices,
                                 const uint64_t* const* cell_indices, const uint64_t* n_cells, const uint8_t* const* const* cells,
                                 const uint64_t* n_proofs, const uint8_t* const* const* proofs, bool leaf) {
        VerifyManyInput in;
        in.n_commitments = n_commitments; in.n_indices = n_indices; in.n_cells = n_cells; in.n_proofs = n_proofs;
        in.commitments = commitments; in.cell_indices = cell_indices; in.cells = cells; in.proofs = proofs; in.leaf = leaf;
        return in;
    }
    static VerifyManyInput flat_device(const uint64_t* cell_starts, const uint8_t* d_commitments, const uint64_t* d_cell_indices,
                                       const uint8_t* d_cells, const uint8_t* d_proofs, hipStream_t user_stream, bool leaf) {
        VerifyManyInput in;
        in.cell_starts = cell_starts; in.d_commitments = d_commitments; in.d_cell_indices = d_cell_indices; in.d_cells = d_cells; in.d_proofs = d_proofs;
        in.user_stream = user_stream; in.leaf = leaf;
        return in;
    }
    static VerifyManyInput host_columns(uint64_t n_blobs, const uint8_t* const* commitments, const uint64_t* column_indices,
                                        const uint8_t* const* const* cells, const uint8_t* const* const* proofs, bool leaf) {
        VerifyManyInput in = lists(nullptr, nullptr, nullptr, nullptr, nullptr, cells, nullptr, proofs, leaf);
        in.columns = true; in.col_blobs = n_blobs; in.col_commitments = commitments; in.col_indices = column_indices;
        return in;
    }
    static VerifyManyInput device_columns(uint64_t n_blobs, const uint8_t* d_commitments, const uint64_t* column_indices, const uint8_t* d_cells,
                                          const uint8_t* d_proofs, hipStream_t user_stream, bool leaf) {
        VerifyManyInput in = flat_device(nullptr, d_commitments, nullptr, d_cells, d_proofs, user_stream, leaf);
        in.columns = in.col_device = true; in.col_blobs = n_blobs; in.col_indices = column_indices;
        return in;
    }
    // partial columns: a bitmap of the blobs present per column (verify_host.hpp: PartialColumns, made by the caller once per call);
    // cells[b][k] / proofs[b][k] on the host, or d_cells / d_proofs packed column after column from part.start[b] on.  Defined in
    // verify_many.hip, where PartialColumns is complete: n_blobs and the counts are taken from `part` there and nowhere else
    static VerifyManyInput host_partial_columns(const PartialColumns& part, const uint8_t* const* commitments, const uint64_t* column_indices,
                                                const uint8_t* const* const* cells, const uint8_t* const* const* proofs, bool leaf);
    static VerifyManyInput device_partial_columns(const PartialColumns& part, const uint8_t* d_commitments, const uint64_t* column_indices,
                                                  const uint8_t* d_cells, const uint8_t* d_proofs, hipStream_t user_stream, bool leaf);
    static VerifyManyInput host_blobs(const uint8_t* const* blobs, const uint8_t* const* commitments, const uint8_t* const* const* proofs) {
        VerifyManyInput in = lists(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, proofs, /*leaf=*/true);
        in.from_blobs = true; in.blobs = blobs; in.blob_commitments = commitments;
        return in;
    }
    static VerifyManyInput device_blobs(const uint8_t* d_blobs, const uint8_t* d_commitments, const uint8_t* d_proofs, hipStream_t user_stream) {
        VerifyManyInput in = flat_device(nullptr, d_commitments, nullptr, nullptr, d_proofs, user_stream, /*leaf=*/true);
        in.from_blobs = in.blobs_device = true; in.d_blobs = d_blobs;
        return in;
    }
    bool on_device() const { return from_blobs ? blobs_device : columns ? col_device : cell_starts != nullptr; }
    uint64_t cells_of(uint64_t b) const {
        if (part) return part_count[part_base + (col_place ? col_place[b] : b)];  // m_b
        return from_blobs ? 128 : columns ? col_blobs : on_device() ? cell_starts[b + 1] - cell_starts[b] : n_cells[b];
    }
    VerifyManyInput from(uint64_t lo) const {  // the problems from lo on (the flat arrays stay: cell_starts holds absolute entries)
        VerifyManyInput s = *this;
        if (from_blobs) {  // (one entry per blob in every array: the arrays themselves move)
            if (blobs_device) { s.d_blobs += lo * 131072; s.d_commitments += lo * 48; s.d_proofs += lo * 128 * 48; }
            else { s.blobs += lo; s.blob_commitments += lo; s.proofs += lo; }
            s.out.first += lo;
            return s;
        }
        if (columns) {
            if (col_place) { s.col_place += lo; return s; }
            // before the places are made ONLY the host form may be cut: nothing here carries an offset into d_cells / d_proofs
            s.col_indices += lo;  // (cells and proofs may be null when there are no blobs)
            s.part_base += lo;
            if (cells && proofs) { s.cells += lo; s.proofs += lo; }
            return s;
        }
        if (on_device()) { s.cell_starts += lo; return s; }
        s.n_commitments += lo; s.n_indices += lo; s.n_cells += lo; s.n_proofs += lo;
        s.commitments += lo; s.cell_indices += lo; s.cells += lo; s.proofs += lo;
        return s;
    }
};

// Many verify_kzg_proof items in one call (point_many.hip; the statement: verify_host.hpp, PointProofTranscript).  Two sources:
//   pointer lists on the host: commitments[i] / proofs[i] -> 48 bytes, zs[i] / ys[i] -> 32 bytes big-endian
//   flat arrays in this GPU's HBM (on_device): n x 48 / n x 32 bytes; the 48-byte arrays from any byte address, zs and ys 4-byte
//     aligned; what user_stream has queued produces them
// A third source, BLOBS (from_blobs; eth_kzg_amd_verify_blob_kzg_proof_many / _many_device): the item is (blob, commitment, proof) and the
// pass computes z = blob_challenge(blob, commitment) and y = p(z) itself (verify_host.hpp); zs / ys are not given.  blobs[i] -> 131072
// bytes on the host, or d_blobs: n x 131072 bytes in HBM, 4-byte aligned, read where they lie.
struct PointManyInput {
    const uint8_t *const *commitments = nullptr, *const *zs = nullptr, *const *ys = nullptr, *const *proofs = nullptr;
    const uint8_t *d_commitments = nullptr, *d_zs = nullptr, *d_ys = nullptr, *d_proofs = nullptr;
    const uint8_t* const* blobs = nullptr;
    const uint8_t* d_blobs = nullptr;
    bool on_device = false, from_blobs = false;
    hipStream_t user_stream = nullptr;
    PointManyInput from(uint64_t lo) const {
        PointManyInput s = *this;
        if (on_device) {
            s.d_commitments += lo * 48; s.d_proofs += lo * 48;
            if (from_blobs) s.d_blobs += lo * 131072;
            else { s.d_zs += lo * 32; s.d_ys += lo * 32; }
        } else {
            s.commitments += lo; s.proofs += lo;
            if (from_blobs) s.blobs += lo;
            else { s.zs += lo; s.ys += lo; }
        }
        return s;
    }
};
// Tap of such a call (null in every product call; the stage hook test_verify_kzg_proof_many_sums sets it): copies of what the passes'
// pinned read-backs held after the syncs they make anyway.  pass_size: 0 = the product's (POINT_MANY_PASS; BLOB_MANY_PASS for the blob
// source), else a forced one.
struct PointManyTap {
    int pass_size = 0;
    std::vector<uint8_t> zs, ys;         // [n][32] each, the blob source only: the z and y the pass computed, as its leaves hash them
    std::vector<uint64_t> pass_starts;   // the first item of every pass, then n
    std::vector<uint8_t> leaves;         // [n][32]
    std::vector<uint8_t> seeds;          // [passes][32]
    std::vector<uint32_t> rho;           // [n][4], as uploaded
    std::vector<uint8_t> fold;           // [passes][2] JacQ: the full-range pair
    std::vector<int> fold_verdict;       // [passes]
    std::vector<int> probes;             // the searches' probes in order: pass, lo, hi (positions in the pass), passed
    std::vector<uint8_t> probe_sums;     // [probe][2] JacQ
    int device_probes = 0;               // probes whose pairing ran on the GPU (k_pairing_check); the others ran on the host threads
};

// How a single cell verification takes its Fiat-Shamir challenge (verify.hip).  Null or `leaf` false: the reference's transcript, one
// SHA-256 over the whole batch on a host core.  leaf: the leaf-hashed challenge (verify_host.hpp: CellLeafTranscript) -- one SHA-256
// per cell on the GPU, out of the arena the inputs are staged into anyway, and one short SHA-256 over the digests on the host.
// The two taps are null in every product call (the stage hooks set them).
struct CellChallengeMode {
    bool leaf = false;
    uint8_t* digest_out = nullptr;  // the 32 bytes r was reduced from
    uint8_t* leaves_out = nullptr;  // (leaf) the n x 32 leaf digests as they came down; the call then returns OK behind them, before any verdict is read
};

enum Status : int {
    OK = 0,
    ERR_SCALAR = 1,    // a field element >= r   (SerializationError::CouldNotDeserializeScalar)
    ERR_G1 = 2,        // bad G1 encoding / not on curve / not in subgroup
    ERR_INPUT = 3,     // length / index validation failed
    ERR_RECOVERY = 4,  // recovered polynomial has non-zero high coefficients
    ERR_DEVICE = 5,    // HIP failure
    ERR_COMMITMENT = 6,  // checked recovery: the recovered polynomial's commitment differs from the one given (public; 5 is internal)
};

// Scoped scratch buffers of the host-pointer entry points come from per-context pools instead of hipMalloc / hipFree
// (both cost 0.1 - 1 ms and hipFree drains the device): blocks are kept by power-of-two size class and reused; the pool
// is emptied with the context.  Callers hold Engine::mu_, so no locking here.
class BufferPool {
public:
    explicit BufferPool(bool pinned_host) : host_(pinned_host) {}
    ~BufferPool();
    void* get(size_t bytes, size_t* cls);
    void put(void* p, size_t cls);
private:
    bool host_;
    std::vector<std::pair<size_t, void*>> free_;
    size_t pooled_ = 0;
};
class Engine;
struct PoolBuf {  // RAII: a block of at least `bytes` from the context's device (or pinned-host) pool
    void* p = nullptr;
    PoolBuf(Engine& e, size_t bytes, bool pinned_host = false);
    ~PoolBuf();
    PoolBuf(const PoolBuf&) = delete;
    PoolBuf& operator=(const PoolBuf&) = delete;
private:
    Engine& e_;
    size_t cls_ = 0;
    bool host_;
};

// One set of device scratch for a prover call: coefficients, MSM scalars, G1 arrays, status words, the staging buffers of
// the host-pointer entry point and the streams / events that order its use.  The engine owns a few of them, so that
// independent calls (and the chunks of one large host-pointer call) overlap on the GPU instead of queueing on one lock.
struct Work {
    std::mutex mu;  // held while a call enqueues on / owns this set
    int cap = 0;    // blobs the arrays below hold
    void *coeffs = nullptr, *canon = nullptr, *scalars = nullptr, *X = nullptr;
    int* status = nullptr;
    void *circ_table = nullptr, *slp_arena = nullptr;
    size_t slp_arena_bytes = 0;
    hipEvent_t done = nullptr;  // recorded after the last kernel that touches the set; the next user's stream waits on it
    // host-pointer path: device and pinned-host staging for one chunk, a compute stream, a copy stream, events
    int stage_cap = 0;
    uint8_t *d_in = nullptr, *d_cells = nullptr, *d_proofs = nullptr;
    uint8_t *h_in = nullptr, *h_cells = nullptr, *h_proofs = nullptr;
    int* h_status = nullptr;
    hipStream_t stream = nullptr, copy = nullptr;
    hipEvent_t ev_in = nullptr, ev_cells = nullptr, ev_cells_host = nullptr, ev_done = nullptr;
    hipEvent_t ev_coeffs = nullptr, ev_side = nullptr;  // small batches: coefficients ready / cells written on the second stream
    std::vector<hipEvent_t> sub_events;  // per sub-batch of a host-pointer call: [2i] cells computed, [2i+1] cells on the host
    // the column prover (data_columns.hip), which commits from the same decode as it proves: canonical coefficients (128 KB per blob) and
    // the commitment MSM's 64 sums per blob, grown on first use; the commitments' staging of its host form
    int col_cap = 0;
    void *col_canon = nullptr, *col_sums = nullptr;
    int comm_cap = 0;
    uint8_t *d_comm = nullptr, *h_comm = nullptr;
    // blobs_to_data_columns (data_columns.hip), which uses nothing of the set but its streams and events: its own status words
    int sc_cap = 0;
    int* sc_status = nullptr;
};
// (HostPool, the combiner, pass-slot and lane leases: host_sync.hpp -- HIP-free, driven under ThreadSanitizer on the CPU)
class Engine {
public:
    friend struct PoolBuf;
    struct SharedTable;  // engine.hip
    // use_precomp: true -> the widest GLV window tables inside the budget (engine_tables.hip: build_final_tables; the reference's
    //              UsePrecomp::Yes uses width 8 on the CPU), false -> the sixteen-window tables only (2.4 GB, twice the additions of
    //              eight windows).  Results identical.  Tables are shared by the contexts of a device.
    // primary: the context's engine when this one is an auxiliary lane of it (lease_serial): the lane shares the primary's
    // window tables by reading through to its view -- no registry look-up, no builder thread, no lock shared with a build
    // table_budget_gb: > 0: upper bound for both window tables together; 0: $ETH_KZG_AMD_TABLE_GB, else DEFAULT_TABLE_BUDGET_GB;
    // < 0: whatever the HBM still holds
    // setup: the trusted setup the context is built on (trusted_setup.hpp); null: the mainnet ceremony file linked into the library.
    // A lane takes its primary's.  Only what is a function of the setup is derived from it (the decompressed points, beta's
    // self-test, the FK20 bases, the window tables, the prepared G2 points): twiddles, linear-map programs and NAF tables are not.
    Engine(bool use_precomp, int device, const Engine* primary = nullptr, double table_budget_gb = 0,
           std::shared_ptr<const TrustedSetup> setup = nullptr);
    // The default memory budget of the window tables: the nine-window GLV tables (nominal width 15: two windows of 15 bits and seven
    // of 14, 18 gathered additions per base) for FK20 (70.9 GB) and for the commitments (35.4 GB).  Measured on one box, same
    // resident 2048-blob batch: -8 % against the widest FK20 table (eight windows of 16 bits: 206 GB) at 43 % of the memory; the next
    // step down (ten windows, 29 GB) costs another 6 %.  Taking "whatever HBM holds" is a decision for the host application
    // (ETH_KZG_AMD_TABLE_GB=max, or the budget argument of eth_kzg_amd_das_context_try_new).
    static constexpr double DEFAULT_TABLE_BUDGET_GB = 108.0;
    ~Engine();
    Engine(const Engine&) = delete;

    // The verification / recovery / commitment / EIP-4844 entry points serialise on one lock per Engine (they share its stream
    // and scratch).  So that calls from different host threads overlap, as they do on the reference's immutable context
    // (bindings/node/src/lib.rs:92-299), the context keeps up to ETH_KZG_AMD_SERIAL_LANES (default 4) engines: the primary one
    // and auxiliaries created on demand (0.1 s each; the window tables are shared, so no memory to speak of).  lease_serial()
    // hands out a free one -- the primary when it is idle -- and blocks only when all are busy.
    using SerialLease = LanePool<Engine>::Lease;  // {Engine* e; std::unique_lock<std::mutex> busy;}
    friend class LanePool<Engine>;

    SerialLease lease_serial();

    int device() const { return dev_; }
    const TrustedSetup& setup() const { return *setup_; }
    Comm* comm() const { return comm_; }       // RCCL communicator attached by eth_kzg_amd_comm_init (multi_gpu.cpp)
    void set_comm(Comm* c) { comm_ = c; }
    hipStream_t stream() const { return stream_; }
    const std::string& last_error() const;  // of the calling thread's last failed call

    // ---- device-resident batch entry points (flat buffers in HBM, launched on `stream`) ----
    // d_blobs: n * 131072 B.  d_cells: n * 128 * 2048 B.  d_proofs: n * 128 * 48 B.  d_commitments: n * 48 B.
    // h_status: n ints (host), 0 = ok.  Any output pointer may be null to skip that product.
    int compute_cells_and_kzg_proofs_device(int n, const uint8_t* d_blobs, uint8_t* d_cells, uint8_t* d_proofs,
                                            int* h_status, hipStream_t stream, bool sync);
    int blob_to_kzg_commitment_device(int n, const uint8_t* d_blobs, uint8_t* d_commitments, int* h_status,
                                      hipStream_t stream, bool sync);

    // ---- a block's data columns in column layout (data_columns.hip; c_eth_kzg.h: eth_kzg_amd_compute_data_columns / _recover_data_columns) ----
    // The prover's call: d_commitments n * 48 B, d_cells [128][n][2048], d_proofs [128][n][48], each may be null.  One decode per
    // sub-batch feeds the commitment and the proofs; status, stream and sync rules of compute_cells_and_kzg_proofs_device.
    int compute_data_columns_device(int n, const uint8_t* d_blobs, uint8_t* d_commitments, uint8_t* d_cells, uint8_t* d_proofs, int* h_status,
                                    hipStream_t stream, bool sync);
    // host pointers: blobs [lo, lo + n) of the caller's arrays (a slice of the call: the arrays are the WHOLE call's, out_cells[c][i] with
    // i a blob of the call); h_status: the whole call's as well.  Outputs of a refused blob are left untouched.
    int compute_data_columns_host(int lo, int n, const uint8_t* const* blobs, uint8_t* const* out_commitments, uint8_t* const* const* out_cells,
                                  uint8_t* const* const* out_proofs, int* h_status);
    // The call of a node that HOLDS the proofs (c_eth_kzg.h: eth_kzg_amd_blobs_to_data_columns without its flag; the flagged forms are an
    // output of the many-verification's blob source, VerifyManyInput::out): d_cells [128][n][2048] straight from k_blob_to_columns,
    // d_out_proofs [128][n][48] = d_proofs [n][128][48] re-ordered, each may be null; status, stream and sync rules of
    // compute_data_columns_device.  Uses none of the prover's workspace.  Host form: the slice [lo, lo + n) of the whole call's arrays;
    // every blob goes up once, only cells 64..127 come down, the rest is copied on the host from the caller's own bytes.
    int blobs_to_data_columns_device(int n, const uint8_t* d_blobs, const uint8_t* d_proofs, uint8_t* d_cells, uint8_t* d_out_proofs, int* h_status,
                                     hipStream_t stream, bool sync);
    int blobs_to_data_columns_host(int lo, int n, const uint8_t* const* blobs, const uint8_t* const* const* proofs, uint8_t* const* const* out_cells,
                                   uint8_t* const* const* out_proofs, int* h_status);
    // The supernode's call: all 128 columns of R blobs from n_columns of them.  d_cells [n_columns][R][2048] in HBM, column_indices on the
    // host; outputs as above.  ONE vanishing polynomial per call.  A bad list marks every blob ERR_INPUT before anything is launched.
    int recover_data_columns_device(int R, uint64_t n_columns, const uint64_t* column_indices, const uint8_t* d_cells, uint8_t* d_out_cells,
                                    uint8_t* d_out_proofs, int* status, hipStream_t stream);
    // host pointers: cells[j][i], blobs [lo, lo + R) of the call; out_cells / out_proofs [128][blobs of the call], may be null; status: the whole call's
    int recover_data_columns_host(int lo, int R, uint64_t n_columns, const uint64_t* column_indices, const uint8_t* const* const* cells,
                                  uint8_t* const* const* out_cells, uint8_t* const* const* out_proofs, int* status);
    // The same recovery checked against the block's commitments (c_eth_kzg.h: eth_kzg_amd_recover_data_columns_checked): what the checked
    // forms add to the two calls above, which are these with an empty RecoverCheck.  Device form: d_* in HBM at any byte address,
    // d_commitments / d_out_commitments R * 48, d_out_blobs [R][131072]; host form: the whole call's pointer arrays, indexed lo + r.
    // Each may be null.  A blob whose commitment differs gets ERR_COMMITMENT behind ERR_SCALAR and ERR_RECOVERY.
    struct RecoverCheck {
        const uint8_t* d_commitments = nullptr;
        uint8_t *d_out_blobs = nullptr, *d_out_commitments = nullptr;
        const uint8_t* const* commitments = nullptr;
        uint8_t* const* out_blobs = nullptr;
        uint8_t* const* out_commitments = nullptr;
        bool commits() const { return d_commitments || d_out_commitments || commitments || out_commitments; }
    };
    int recover_data_columns_checked_device(int R, uint64_t n_columns, const uint64_t* column_indices, const uint8_t* d_cells, const RecoverCheck& chk,
                                            uint8_t* d_out_cells, uint8_t* d_out_proofs, int* status, hipStream_t stream);
    int recover_data_columns_checked_host(int lo, int R, uint64_t n_columns, const uint64_t* column_indices, const uint8_t* const* const* cells,
                                          const RecoverCheck& chk, uint8_t* const* const* out_cells, uint8_t* const* const* out_proofs, int* status);

    // ---- host-buffer entry points (what the reference's C ABI hands over) ----
    int compute_cells_and_kzg_proofs_host(int n, const uint8_t* const* blobs, uint8_t* const* const* cells,
                                          uint8_t* const* const* proofs, int* h_status);
    int blob_to_kzg_commitment_host(int n, const uint8_t* const* blobs, uint8_t* const* out, int* h_status);

    // verify_cell_kzg_proof_batch (eip7594/src/verifier.rs:72-112): returns a Status; *verified set on OK.
    int verify_cell_kzg_proof_batch_host(uint64_t n_commitments, const uint8_t* const* commitments, uint64_t n_indices,
                                         const uint64_t* cell_indices, uint64_t n_cells, const uint8_t* const* cells,
                                         uint64_t n_proofs, const uint8_t* const* proofs, int* verified, const CellChallengeMode* mode = nullptr);
    // the same check on flat arrays in this GPU's HBM: n * 48 commitment bytes (one per cell, not deduplicated), n u64 indices,
    // n * 2048 cell bytes, n * 48 proof bytes.  With the leaf-hashed challenge neither cells nor proofs come down: only the
    // commitments and the indices (validation, de-duplication) and the n * 32 leaf digests do
    int verify_cell_kzg_proof_batch_device(uint64_t n, const uint8_t* d_commitments, const uint64_t* d_cell_indices,
                                           const uint8_t* d_cells, const uint8_t* d_proofs, int* verified, hipStream_t stream,
                                           const CellChallengeMode* mode = nullptr);
    // MANY independent verifications in one call (verify_many.hip), from any source and with either challenge (VerifyManyInput above):
    // status[b] = a Status (OK, ERR_INPUT, ERR_G1, ERR_SCALAR), verified[b] set when OK.  Returns ERR_DEVICE on a HIP failure, OK
    // otherwise.  Does not take mu_: runs next to the other entry points.
    int verify_cell_kzg_proof_batch_many(uint64_t n_batches, const VerifyManyInput& in, int* verified, int* status, VerifyManyTap* tap = nullptr);
    // verify_cell_kzg_proof_batch as the reference's users call it -- one problem per call, from many threads on one context
    // (bindings/node/src/lib.rs:92-299) -- WITHOUT asking them to batch: the first callers take the latency-optimised path
    // (verify_cell_kzg_proof_batch_host, one per engine lane); callers that arrive while every lane is verifying
    // are COMBINED: they queue their problems, one of them becomes the leader and runs everything queued as one
    // many-verification pass, the others sleep until their verdict is in.  Same verdicts and error split as the single path.
    int verify_cell_kzg_proof_batch_combined(uint64_t n_commitments, const uint8_t* const* commitments, uint64_t n_indices,
                                             const uint64_t* cell_indices, uint64_t n_cells, const uint8_t* const* cells,
                                             uint64_t n_proofs, const uint8_t* const* proofs, int* verified);
    // the same check sharded over ranks: every rank passes the WHOLE batch (the Fiat-Shamir transcript covers it) and its
    // slice [lo, hi) of the cell list, gets 96 bytes back; the gathered records go to _combine on any rank.
    int verify_cell_kzg_proof_batch_partial_host(uint64_t n_commitments, const uint8_t* const* commitments, uint64_t n_indices,
                                                 const uint64_t* cell_indices, uint64_t n_cells, const uint8_t* const* cells,
                                                 uint64_t n_proofs, const uint8_t* const* proofs, uint64_t lo, uint64_t hi,
                                                 uint8_t* out96);
    int verify_cell_kzg_proof_batch_combine_host(uint64_t n_partials, const uint8_t* partials96, int* verified);
    // recover_cells_and_kzg_proofs (eip7594/src/prover.rs:156-171)
    int recover_cells_and_kzg_proofs_host(uint64_t n_cells, const uint8_t* const* cells, uint64_t n_indices,
                                          const uint64_t* cell_indices, uint8_t* const* out_cells,
                                          uint8_t* const* out_proofs);

    // EIP-4844 single-point operations (crates/eip4844/src/{prover,verifier}.rs); Status returns
    int compute_kzg_proof_host(const uint8_t* blob, const uint8_t* z, uint8_t* out_proof, uint8_t* out_y);
    int compute_blob_kzg_proof_host(const uint8_t* blob, const uint8_t* commitment, uint8_t* out_proof);
    int verify_kzg_proof_host(const uint8_t* commitment, const uint8_t* z, const uint8_t* y, const uint8_t* proof, int* verified);
    int verify_blob_kzg_proof_host(const uint8_t* blob, const uint8_t* commitment, const uint8_t* proof, int* verified);
    // sums2 (here and in the device form; null in every product call): receives the two sums the pairing check pairs, rhs then lhs
    int verify_blob_kzg_proof_batch_host(uint64_t n_blobs, const uint8_t* const* blobs, uint64_t n_commitments,
                                         const uint8_t* const* commitments, uint64_t n_proofs, const uint8_t* const* proofs,
                                         int* verified, G1Affine* sums2 = nullptr);
    // MANY verify_kzg_proof items in one call, a verdict each (point_many.hip): status[i] = ERR_G1 / ERR_SCALAR / OK in the single
    // call's order of checks, verified[i] set when OK.  Returns ERR_DEVICE on a HIP failure, OK otherwise.  Runs on a pass slot of the
    // many-verification: does not take mu_.
    // in.from_blobs: MANY verify_blob_kzg_proof items, status[i] = ERR_SCALAR (the blob) / ERR_G1 / OK in that call's order.
    int verify_kzg_proof_many(uint64_t n, const PointManyInput& in, int* verified, int* status, PointManyTap* tap = nullptr);
    // ---- EIP-4844 proofs for MANY blobs (eip4844.hip; crates/eip4844/src/prover.rs:37-92 per blob) ----
    // Device-resident: d_blobs n * 131072 B, d_commitments / d_out_proofs n * 48 B, d_z / d_out_y n * 32 B big-endian (4-byte aligned);
    // h_status: n ints on the host or null.  status per blob in the single call's order: 1 the blob holds a non-canonical element,
    // else 1 z is not canonical (compute_kzg_proof) / 2 the commitment is not a valid subgroup point (compute_blob_kzg_proof), else 0.
    // Stream, event and status == null rules as blob_to_kzg_commitment_device.  The Fiat-Shamir challenges of the blob proofs are
    // hashed on the GPU (k_sha256.hip): the blobs do not come down.
    int compute_blob_kzg_proof_device(int n, const uint8_t* d_blobs, const uint8_t* d_commitments, uint8_t* d_out_proofs, int* h_status,
                                      hipStream_t stream, bool sync);
    int compute_kzg_proof_device(int n, const uint8_t* d_blobs, const uint8_t* d_z, uint8_t* d_out_proofs, uint8_t* d_out_y, int* h_status,
                                 hipStream_t stream, bool sync);
    // host pointers: blobs gathered into pinned memory and challenges hashed by the helper threads, one upload and one opening per
    // sub-batch of 256 blobs; outputs of a blob whose status is not 0 are left untouched
    int compute_blob_kzg_proof_batch_host(int n, const uint8_t* const* blobs, const uint8_t* const* commitments, uint8_t* const* out_proofs,
                                          int* h_status);
    int compute_kzg_proof_batch_host(int n, const uint8_t* const* blobs, const uint8_t* const* zs, uint8_t* const* out_proofs,
                                     uint8_t* const* out_ys, int* h_status);
    // verify_blob_kzg_proof_batch (verifier.rs:80-196) on flat arrays in HBM: challenges and evaluations on the GPU, points decompressed
    // where they lie; the n * 160 bytes of the weights' transcript come down.  Synchronous; verdict and error split of the host form.
    int verify_blob_kzg_proof_batch_device(uint64_t n, const uint8_t* d_blobs, const uint8_t* d_commitments, const uint8_t* d_proofs,
                                           int* verified, hipStream_t stream, G1Affine* sums2 = nullptr);

    // device-resident recovery: flat [R][128][2048] cells in HBM + a 128-bit presence mask per blob (host); see verify.hip
    int recover_cells_and_kzg_proofs_device(int R, const uint8_t* d_cells, const uint64_t* present_masks, uint8_t* d_out_cells,
                                            uint8_t* d_out_proofs, int* status, hipStream_t stream);
    // batched form: R independent recoveries in one pass (ragged cell lists); status[r] per blob
    int recover_cells_and_kzg_proofs_batch_host(int R, const uint64_t* n_cells, const uint8_t* const* const* cells,
                                                const uint64_t* n_indices, const uint64_t* const* cell_indices,
                                                uint8_t* const* const* out_cells, uint8_t* const* const* out_proofs,
                                                int* status);

    // ---- stage-level hooks for the kernel parity tests (host buffers, canonical encodings) ----
    int test_fr_ntt4096(const uint8_t* in_be, uint8_t* out_be, int inverse_dit);
    int test_g1_fft128(const uint8_t* in_compressed, uint8_t* out_compressed, int n_lanes, int inverse);
    int test_fixed_msm(const uint8_t* scalars_be, int n_msm, uint8_t* out_compressed);
    // one stated schedule of the fixed-base MSM on either window table (engine_testhooks.hip); modes5: the launches made, then their modes
    int test_fixed_msm_ex(int table_kind, int mode, int scalar_form, const uint8_t* scalars, int n_slices, uint8_t* out_compressed, int32_t* modes5);
    // enqueue_compute on n blobs (host), then the MSM scalars it left in the work set: segs x n x 8192 x 8 words, as launch_msm reads them
    int test_prover_scalars(int n, const uint8_t* blobs, uint32_t* scalars, uint64_t max_words, uint64_t* n_words, uint8_t* cells, uint8_t* proofs,
                            int32_t* status, int32_t* fused_launches);
    // the G1 stage alone: prepare_g1_stage / run_g1_stage (engine_prover.hip) around sums the caller gives as raw JacS words
    int test_proofs_from_sums(int program, int n, const int32_t* sums_words, uint8_t* out_proofs);
    // what was uploaded for a compilation of the linear map: its words (read back from the device), launches, slots, constants
    int test_linmap_program(int program, uint32_t* words, uint64_t max_words, uint64_t* n_words, int32_t* launches3, uint64_t max_launches,
                            uint64_t* n_launches, int32_t* n_slots, uint8_t* consts_be, uint64_t max_consts, uint64_t* n_consts);
    int test_g1_decompress(const uint8_t* in, int n, int subgroup_check, int* h_status, uint8_t* out_recompressed);
    // the decoded affine coordinates behind each decode / subgroup launch call (form 0 .. 4: engine_testhooks.hip), segments [n0 | n1]
    int test_g1_decode(int form, const uint8_t* in, int n0, int n1, int32_t* h_status, uint8_t* out_xy);
    int test_field_mul(const uint8_t* a, const uint8_t* b, uint8_t* out, int n, int is_fp);
    int test_op(int op, int n, const int32_t* in, int32_t* out);
    // launch::sha256_many on its own: prefix on the host, every other buffer in HBM
    int test_sha256_many(int n, const uint8_t* prefix, uint32_t prefix_len, const uint8_t* d_body, size_t body_stride, uint32_t body_len,
                         const uint8_t* d_tail, size_t tail_stride, uint32_t tail_len, uint8_t* d_out);
    // the verifier's two-job bucket MSM on its own (k_verify.hip).  form: 0 windowed, 1 byte-shifted after pip_shift_prepare, 2 byte-shifted
    // after pip_shift_prepare_and_subgroup as verify.hip launches it; h_status (n_pts ints, may be null): the points' status words
    int test_verify_msm(int form, const uint8_t* points, int n_pts, const uint8_t* sc0_be, int n0, const uint8_t* sc1_be, int n1,
                        uint8_t* out96, int32_t* h_status);
    // the two pairing inputs of the cells [lo, hi) of a device-resident batch, compressed: verify_cells_partial behind the set-up of
    // verify_cell_kzg_proof_batch_device (verify_cells_partial_device: the pinned mirror in chunks, the device source)
    int test_verify_cells_partial_device(uint64_t n, const uint8_t* d_commitments, const uint64_t* d_cell_indices, const uint8_t* d_cells,
                                         const uint8_t* d_proofs, uint64_t lo, uint64_t hi, uint8_t* out96);
    // the leaf digests of a batch given as flat host arrays, by the staging and the launch the leaf-hashed verification makes (verify.hip)
    int test_cell_leaf_digests(uint64_t n, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs,
                               uint8_t* out_digests);
    // the whole batch's challenge digest and two pairing inputs under either transcript (flags: ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT or 0);
    // on_device: the flat arrays of the device-resident form, else the host form's pointer arrays
    int test_verify_cells_inputs_ex(uint64_t n, int on_device, const void* commitments, const void* cell_indices, const void* cells,
                                    const void* proofs, uint32_t flags, uint8_t* root32, uint8_t* out96);
    // the two sums verify_blob_kzg_proof_batch pairs (rhs | lhs, compressed) and its verdict; on_device: flat arrays in HBM, else host pointers
    int test_verify_blob_batch_inputs(uint64_t n, int on_device, const void* blobs, const void* commitments, const void* proofs, uint8_t* out96,
                                      int* verified);
    // one pass of verify_cell_kzg_proof_batch_many with its tap set: verdicts and statuses as the call gives them, form = small, folded,
    // searched, folded verdict; sums96[B] and fold96 compressed on the host from the sums read back, rho[B][4], the search's probes
    // (probe_ranges[i] = lo, hi, passed; probe_sums96[i]) up to max_probes of them, *n_probes = how many there were
    // over any source and with either challenge (VerifyManyInput), plus digests32[B][32], may be null (the digest each problem's challenge was reduced
    // from; zero for a problem that was not hashed) and, may be null, leaves32[N][32] (leaf-hashed challenges: the leaf digests in the
    // caller's cell order; zero for the cells of a problem that was not hashed)
    int test_verify_many_sums_in(uint64_t n_batches, const VerifyManyInput& in, int32_t* verified, int32_t* status, int32_t* form4, uint8_t* sums96,
                                 uint32_t* rho, uint8_t* fold96, int32_t* probe_ranges, uint8_t* probe_sums96, uint64_t max_probes, uint64_t* n_probes,
                                 uint8_t* digests32, uint8_t* leaves32, uint64_t* counts2 = nullptr);
    // (counts2, may be null: the commitment points the pass decoded and the scalar multiplications it launched, VerifyManyTap)
    // verify_kzg_proof_many with its tap set and, if forced_pass > 0, passes of that many items: verdicts and statuses as the call gives
    // them, the pass bounds (pass_starts: up to max_passes + 1 entries), leaves32[n][32], seeds32 / fold96 / fold_verdicts per pass,
    // rho[n][4], the probes (probes4[i] = pass, lo, hi, passed; probe_sums96[i]) up to max_probes of them; pairs compressed on the host
    int test_verify_kzg_proof_many_sums(uint64_t n, const PointManyInput& in, uint64_t forced_pass, int32_t* verified, int32_t* status,
                                        uint64_t* pass_starts, uint64_t max_passes, uint64_t* n_passes, uint8_t* leaves32, uint8_t* seeds32, uint32_t* rho,
                                        uint8_t* fold96, int32_t* fold_verdicts, int32_t* probes4, uint8_t* probe_sums96, uint64_t max_probes,
                                        uint64_t* n_probes, uint8_t* zs32 = nullptr, uint8_t* ys32 = nullptr /* the blob source: [n][32] each */);
    // k_blob_eval_at alone: n blobs and n points (32 big-endian bytes, reduced mod r) from the host -> ys32[n][32], bad[n]
    int test_blob_eval_at(int n, const uint8_t* const* blobs, const uint8_t* zs_be32, uint8_t* out_ys_be32, int32_t* out_bad);
    // k_blob_to_extension alone behind the copy of cells 0..63: n blobs from the host -> out_cells[n][128][2048], bad[n] (the status word)
    int test_blob_extension(int n, const uint8_t* const* blobs, uint8_t* out_cells, int32_t* out_bad);
    // k_blob_to_columns alone: n blobs from the host as blobs [b0, b0 + n) of a matrix of n_total; matrix [128][n_total][2048] on the host goes
    // up as it is (the caller's guard pattern), one launch, and comes down; bad[n]: the status words
    int test_blob_to_columns(int n, const uint8_t* const* blobs, uint64_t n_total, uint64_t b0, int blob_half, uint8_t* matrix, int32_t* out_bad);
    // k_pairing_check and the host's checks on the same n pairs (compressed G1, n x 2 x 48 bytes) against key pair `key` (0: [tau^64]_2, -[1]_2;
    // 1: [tau]_2, -[1]_2); flags: see include/c_eth_kzg_test_hooks.h.  The Miller values (may be null): n x 576 bytes each
    int test_pairing_check_many(int key, uint64_t n, const uint8_t* pairs, int flags, int8_t* out_gpu, int8_t* out_host, uint8_t* out_miller_gpu,
                                uint8_t* out_miller_host);
    // out4: probes the last tapped many-verification checked on the GPU, all its probes; nanoseconds of the last test_pairing_check_many on
    // the GPU (launch + verdict copy) and on the host threads
    void test_search_stats(uint64_t* out4) const { for (int i = 0; i < 4; i++) out4[i] = test_search_stats_[i]; }
    uint64_t test_search_stats_[4] = {0, 0, 0, 0};
    // the Reed-Solomon decoder of recovery on its own: rs_decode (verify.hip) with its tap set, behind the staging of recover_batch_to_coeffs
    // (flat_source = 0) or of recover_cells_and_kzg_proofs_device (1); outputs canonical big-endian on the host, each may be null
    int test_rs_decode(int R, const uint64_t* n_cells, const uint64_t* const* cell_indices, const uint8_t* const* const* cells, int flat_source,
                       int32_t* status, int32_t* deg, uint8_t* zp, uint8_t* zeval, uint8_t* zcinv, uint8_t* coeffs);
    // the window tables themselves (engine_testhooks.hip).  kind: TableSel; which: 0 = the complete table the next MSM launch would
    // snapshot (the view's main), 1 = the wider one under construction next to it (its ready groups), 2 = the table the context started on, while it is alive
    std::shared_ptr<SharedTable> test_table(int kind, int which) const;
    int test_table_info(int kind, int which, int64_t* out8, int32_t* piece_first_block, int max_pieces);
    int test_table_audit(int kind, int which, uint64_t* visited, uint64_t* n_findings, int32_t* findings, int max_findings, double* ms);
    int test_table_read(int kind, int which, int group, int window, int base, int d0, int n, uint32_t* out);
    int test_table_audit_buffer(int c, int n_groups, int nb, const uint32_t* table, const uint8_t* bases, uint64_t* visited, uint64_t* n_findings,
                                int32_t* findings, int max_findings);

    // ---- per-stage HIP-event timing (bench.py's roofline leg) ----
    enum Stage { ST_BLOB_TO_COEFFS = 0, ST_COEFFS_TO_CELLS, ST_FK20_SCALARS, ST_MSM_FIXED, ST_G1_IFFT, ST_G1_FFT,
                 ST_COMPRESS, ST_G1_LINMAP, ST_COUNT };
    void set_profiling(bool on);
    // sums since the last call: ms[ST_COUNT], launches[ST_COUNT]; synchronises the device
    void get_stage_times(double* ms, uint64_t* launches);

    // ---- window tables.  A context is usable as soon as its START tables are up (sixteen-window GLV tables: FK20 1.6 GB,
    // commitments 0.8 GB); the wide ones (the widest GLV tables inside the budget: engine_tables.hip, build_final_tables) are
    // built by a helper thread and published with one pointer swap: every MSM launch takes a snapshot of the view, results
    // are identical for every table (tests), only the speed changes.  ETH_KZG_AMD_PROGRESSIVE=0 builds them before the
    // constructor returns.
    struct TableView {  // a snapshot: main = the complete table calls run on, next = a wider one under construction (its
                        // leading ready groups are used already; launch_msm); c / bytes describe main
        std::shared_ptr<SharedTable> main, next;
        int c = 0;          // window width
        size_t bytes = 0;
    };
    enum TableSel { TAB_FK = 0, TAB_SRS = 1 };
    TableView table_view(TableSel which) const;
    // 1 = final tables in place, 0 = still on the start tables (waits up to wait_ms; < 0: until done), 2 = the wide build
    // failed (out of memory ...) and the context stays on what it has
    int tables_ready(int wait_ms);
    // groups of the table under construction that MSMs already run on (all of them once it is complete)
    int table_groups_ready(TableSel which) const;
    // how the tables in use were allocated: out[0] = milliseconds spent in hipMalloc for their pieces (both tables), out[1] = the
    // longest single hipMalloc (ms), out[2] = pieces, out[3] = bytes.  A long single allocation is the driver waiting for memory
    // another process freed to be wiped: the process's GPU queues stand still meanwhile (tools/alloc_test/probe_stall.cpp)
    void table_build_info(double* out4) const;
    void stop_builder();  // abandon an unfinished build of the wide tables and join the helper thread
    size_t table_bytes() const { return table_view(TAB_FK).bytes + table_view(TAB_SRS).bytes; }
    int window_bits() const { return table_view(TAB_FK).c; }  // NOMINAL width of the FK20 table in use: its windows are ceil(128 / c) of mixed widths (launch.hpp)
    int window_count() const { const int c = window_bits(); return c > 0 ? (128 + c - 1) / c : 0; }  // windows per GLV half = gathered additions per base / 2
    const int* linmap_info() const { return slp_info_; }

private:
    void construct();           // the constructor's body; a throw is followed by teardown()
    void teardown() noexcept;   // the destructor's body
    void start_builder();       // progressive start: registers the engine and starts the table builder thread (engine_tables.hip)
    void init_constants();
    void init_linmap(const Fr8* w8192_mont);  // host copy of omega_8192^k
    void init_srs();
    void check_setup_powers();  // TrustedSetup::check_powers: both chains of the setup are powers of one tau (eip4844.hip)
    void settle_streams();
    bool streams_overlap(hipStream_t a, hipStream_t b);
    void init_fk20();
    void init_verifier();
    int open_blobs_at(int n, const uint8_t* const* blobs, const Fr8* z_mont, bool want_proofs, uint8_t* h_proofs, Fr8* h_y_canon,
                      int* h_status);
    // the device-resident core of every opening: blobs in HBM, z_i Montgomery in HBM -> y_i canonical (d_y) and, if d_proofs is not
    // null, proof_i = commit(quotient_i) compressed, all left on the device; the per-blob status words are work_[0]'s (d_status_).
    // Enqueues on st and returns; the caller holds mu_ and has called ensure_workspace(n).
    void open_blobs_core(int n, const uint8_t* d_blobs, const void* d_z_mont, void* d_y, uint8_t* d_proofs, hipStream_t st);
    // scratch of the batched EIP-4844 forms, owned by the engine (grow-only, guarded by mu_; ordered by work_[0].done like the
    // work set): per blob a digest, z, y, the decoded commitment, a proof and three status words
    struct Scratch4844 {
        uint8_t *dig = nullptr, *proofs = nullptr;
        void *z = nullptr, *y = nullptr, *aff = nullptr;
        int *blob_bad = nullptr, *z_bad = nullptr, *g1_bad = nullptr, *status = nullptr;
    };
    Scratch4844 scratch_4844(int n);
    void fs_challenges_device(int n, const uint8_t* d_blobs, const uint8_t* d_commitments, const Scratch4844& s, hipStream_t st);
    int finish_verify_blob_batch(int n, const Fr8* z_mont, const Fr8* y_canon, const uint8_t* const* commitments, const uint8_t* const* proofs,
                                 const void* d_points, G1Affine* sums2 = nullptr);
    // the two host-pointer batch forms (commitments: blob proofs; zs: proofs at given points) and one staged sub-batch of them
    int proofs_batch_host(int n, const uint8_t* const* blobs, const uint8_t* const* commitments, const uint8_t* const* zs,
                          uint8_t* const* out_proofs, uint8_t* const* out_ys, int* h_status);
    void open_staged_blobs(int nb, const uint8_t* h_blobs_pinned, const Fr8* z_mont, const uint8_t* h_commitments, uint8_t* h_proofs, Fr8* h_y,
                           int* h_blob_status, int* h_g1_status);
    HostPool* ensure_host_pool();  // the memcpy / hash helper threads of the host-pointer batch forms (engine_prover.hip)
    void* d_4844_ = nullptr;       // Scratch4844's arena + the 32-byte Fiat-Shamir header in front of it
    int cap_4844_ = 0;
    int pairing_check_4844(const void* d_points, const std::vector<Fr8>& sc0, const std::vector<Fr8>& sc1, G1Affine* sums2 = nullptr);
    // dsrc (device-resident form): the cells and proofs already sit in HBM -- they are copied device to device into the arena
    // instead of being gathered on the host and uploaded; the pointer arrays then address their pinned host mirror, which the
    // transcript hash reads, and whose cells arrive in chunks (an event per chunk)
    // where a single verification stages and computes: the engine's own stream / arena / pinned slab (under mu_), or those of a pass
    // slot (the caller holds the slot): so that up to four single verifications run side by side, each on its own hardware queue
    struct VerifyScratch {
        hipStream_t stream = nullptr;
        void* dev = nullptr;
        size_t dev_cap = 0;
        uint8_t* pin = nullptr;
        size_t pin_cap = 0;
    };
    struct VerifyDeviceSource {
        const uint8_t *d_cells, *d_proofs;  // flat [n][2048] / [n][48] in this GPU's memory
        hipEvent_t* chunk_events;           // chunk j = cells [j * chunk_cells, (j + 1) * chunk_cells) of the mirror
        int chunk_cells, n_chunks;          // (leaf-hashed challenge: no mirror, no chunks: null, 0, 0)
    };
    int verify_cells_partial(uint64_t n_commitments, const uint8_t* const* commitments, uint64_t n_indices,
                             const uint64_t* cell_indices, uint64_t n_cells, const uint8_t* const* cells, uint64_t n_proofs,
                             const uint8_t* const* proofs, uint64_t lo, uint64_t hi, G1Affine* out2, bool* empty,
                             const VerifyDeviceSource* dsrc = nullptr, VerifyScratch* vs = nullptr, const CellChallengeMode* mode = nullptr);
    // the device-resident form's set-up in front of verify_cells_partial: commitments, indices and proofs down into the pinned mirror,
    // the cells behind them in chunks with an event each, the pointer arrays over the mirror, the device source.  The CALLER holds mu_ (the mirror is the context's).
    // Leaf-hashed challenge: commitments and indices only, no mirror of cells or proofs and no chunk events.
    int verify_cells_partial_device(uint64_t n, const uint8_t* d_commitments, const uint64_t* d_cell_indices, const uint8_t* d_cells,
                                    const uint8_t* d_proofs, uint64_t lo, uint64_t hi, G1Affine* out2, bool* empty, hipStream_t user_stream,
                                    const CellChallengeMode* mode = nullptr);
    bool verify_cells_pairing(const G1Affine* pts2) const;
    // the same check with the second pair's Miller loop on a thread of the staging pool (the latency path of a single verification)
    bool verify_cells_pairing_split(const G1Affine* pts2);
    // tap (null in every product call; the stage hook test_rs_decode sets it): host arrays that receive what the decoder's stages left,
    // in the kernels' Montgomery words, before their pool buffers are released -- deg[R], zp[R][65], zeval[R][128], zcinv[R][128]; each may be null
    struct RsDecodeTap { int* deg = nullptr; Fr8 *zp = nullptr, *zeval = nullptr, *zcinv = nullptr; };
    // src_of (null in every call but the column form): list entry k reads cell (*src_of)[k] of d_cells.  shared_pattern (the column form):
    // all R blobs miss the same cells -- `present` holds ONE mask and one vanishing polynomial is built for the call.
    // commit (null in every call but the checked column recovery): behind the decode and in front of its one synchronisation, the
    // commitments of the R recovered polynomials -- the stages of blob_to_kzg_commitment_device on the canonical coefficients the last
    // pass leaves in work_[0].canon, the sums in work_[0].X -- into d_calc (R * 48 bytes of the engine's, 4-byte aligned);
    // d_expected (device, any byte address, or null: nothing is compared): a blob whose 48 bytes differ gets ERR_COMMITMENT unless it
    // has ERR_SCALAR or ERR_RECOVERY already; d_out (device, any address) / h_out (host), each R * 48 bytes or null: copies of d_calc,
    // complete when rs_decode returns.  Every blob runs through the stages, a failed one on whatever its coefficients are.
    struct RsCommit { uint8_t* d_calc = nullptr; const uint8_t* d_expected = nullptr; uint8_t* d_out = nullptr; uint8_t* h_out = nullptr; };
    int rs_decode(int R, const uint8_t* d_cells, bool flat_source, const std::vector<int>& slot, const std::vector<int>& stof,
                  const std::vector<uint32_t>& present, int* st_out, const RsDecodeTap* tap = nullptr, const std::vector<int>* src_of = nullptr,
                  bool shared_pattern = false, const RsCommit* commit = nullptr);
    // the column form's index arrays for blobs [r0, r0 + nr) of n_total, then rs_decode on them (data_columns.hip)
    int rs_decode_columns(int nr, size_t n_total, uint64_t n_columns, const uint64_t* column_indices, const uint8_t* d_cells_r0, int* st_out,
                          const RsCommit* commit = nullptr);
    int recover_batch_to_coeffs(int R, const uint64_t* n_cells, const uint8_t* const* const* cells,
                                const uint64_t* const* cell_indices, int* st_out);
    void ensure_workspace(int n);  // work_[0]; also makes stream_ wait for the last asynchronous call that used it
    void ensure_workspace(Work& w, int n, bool release = false);
    void ensure_staging(Work& w, int n);
    void run_proofs_from_coeffs(int n, uint8_t* d_proofs, hipStream_t st) { run_proofs_from_coeffs(work_[0], n, d_proofs, st); }
    // msm_cut > 0 (host-pointer path, scalars precomputed): the MSM stage in two launches around the cut -- PROOFS_HEAD issues the
    // arena set-up and the MSMs of blobs [0, msm_cut) and returns, PROOFS_TAIL the MSMs of [msm_cut, n) and everything after
    enum ProofsPhase { PROOFS_ALL = 0, PROOFS_HEAD = 1, PROOFS_TAIL = 2 };
    // cols (here and below; null: the blob-major layout): d_cells / d_proofs are the whole call's column arrays (launch::Columns)
    void run_proofs_from_coeffs(Work& w, int n, uint8_t* d_proofs, hipStream_t st, const TableView* tv_pre = nullptr, ProofsPhase phase = PROOFS_ALL,
                                int msm_cut = 0, const launch::Columns* cols = nullptr);
    // d_commitments (the column prover only): the blobs' commitments, n * 48 bytes, from the same decode (enqueue_commitments)
    void enqueue_compute(Work& w, int n, const uint8_t* d_blobs, uint8_t* d_cells, uint8_t* d_proofs, hipStream_t st,
                         hipEvent_t after_cells, const launch::Columns* cols = nullptr, uint8_t* d_commitments = nullptr);
    // the commitment stages of n blobs whose canonical coefficients are in w.col_canon: set_inf, MSM on TAB_SRS, fold, compress
    void enqueue_commitments(Work& w, int n, uint8_t* d_commitments, hipStream_t st);
    void ensure_commit_scratch(Work& w, int n);
    // the body of compute_cells_and_kzg_proofs_device and compute_data_columns_device: sub-batches on one leased work set
    int prover_device(int n, const uint8_t* d_blobs, uint8_t* d_commitments, uint8_t* d_cells, uint8_t* d_proofs, int* h_status, hipStream_t st,
                      bool sync, bool columns);
    // the G1 stage behind the MSM (engine_prover.hip): its program, lanes and point array; then its launches down to the proof bytes
    struct SlpProgram;
    struct G1Stage {
        int bp = 0, segs = 1;
        bool linmap_mode = false;
        const SlpProgram* prog = nullptr;
        int mulc_coop_lanes = 0;  // > 0: so few blobs that the constant multiplications take several lanes per blob (launch::g1_slp_launch)
        void* X = nullptr;        // where the MSM leaves its sums: the linear map's arena, or the work set's point array
        const launch::Columns* cols = nullptr;  // the proofs' layout (null: blob-major)
    };
    G1Stage prepare_g1_stage(Work& w, int n, hipStream_t st, int force_program = -1);
    void run_g1_stage(Work& w, const G1Stage& g, int n, uint8_t* d_proofs, hipStream_t st);
    int fk20_segs(int n) const;  // scaled copies of the scalars the MSM stage of n blobs wants (run_proofs_from_coeffs)
    Work& lease_work(int first, int last);  // locks and returns a free set among work_[first..last] (waits for whichever frees first)
    void release_work(Work& w);
    std::mutex lease_mu_;
    std::condition_variable lease_cv_;
    void set_error(const std::exception& e);
    void launch_msm(const void* scalars, TableSel table, void* out, int n_groups, int n_slices, int out_stride,
                    int brp_bits, hipStream_t st, int out_fmt /* launch::FMT_* */);
    // the stage hook's tap: force >= 0 takes the place of the mode launch_msm_range picks (and of its two-launch overflow form);
    // modes[0 .. n): the mode of every launch::msm_glv call made, in order
    struct MsmTap { int force = -1; int n = 0; int modes[4] = {0, 0, 0, 0}; };
    void launch_msm(const void* scalars, const TableView& tv, bool scalars_split, void* out, int n_groups, int n_slices, int out_stride,
                    int brp_bits, hipStream_t st, int out_fmt /* launch::FMT_* */, MsmTap* tap = nullptr);
    void launch_msm_range(const void* scalars, const SharedTable& t, int g0, int gcnt, void* out, int n_groups, int n_slices, int out_stride,
                          int brp_bits, hipStream_t st, int out_fmt, MsmTap* tap = nullptr);
    long msm_waves(long msms, int c) const;  // waves of the MSM launch launch_msm_range would issue (the side-stream decision of enqueue_compute)
    void build_final_tables();  // the wide tables: on the helper thread (progressive start) or inline
    void publish(TableSel which, const std::shared_ptr<SharedTable>& main, const std::shared_ptr<SharedTable>& next);
    void g1_fft128_full(void* X, int stride, int inverse, hipStream_t st);

    struct StageMark { int stage; int launches; hipEvent_t a, b; };
    int mark_begin(int stage, hipStream_t st);  // -> handle for mark_end (-1 when profiling is off)
    void mark_end(int mark, int launches, hipStream_t st);
    bool profiling_ = false;
    std::vector<StageMark> marks_;
    unsigned marks_gen_ = 0;
    std::mutex marks_mu_;

    int dev_ = 0;
    std::shared_ptr<const TrustedSetup> setup_;  // never null once the constructor's first line has run
    Comm* comm_ = nullptr;
    bool use_precomp_ = true;
    Knobs knobs_;            // every environment knob, read once when the context is created (knobs.hpp)
    int want_glv_c_ = 0;     // ETH_KZG_AMD_GLV_WINDOW: this GLV width exactly (0: the widest that fits memory and budget)
    double table_budget_gb_ = DEFAULT_TABLE_BUDGET_GB;  // upper bound for both tables together (constructor argument, ETH_KZG_AMD_TABLE_GB, or the default); <= 0: what the HBM holds
    mutable std::mutex tab_mu_;
    std::condition_variable tab_cv_;
    std::weak_ptr<SharedTable> start_tab_[2];  // what a progressive start began on (introspection: alive until the wide tables have replaced it)
    Published<SharedTable> pub_[2];  // per table kind: main / next / retired (host_sync.hpp); start tables stay alive for kernels already in flight
    int tables_state_ = 0;  // 0 building, 1 final, 2 wide build failed (guarded by tab_mu_)
    std::string tables_error_;
    std::thread builder_;
    std::atomic<bool> cancel_build_{false};
    bool progressive_build_ = false;  // the wide tables are built next to callers on the start tables: the builder leaves room on the GPU
    hipStream_t build_stream_ = nullptr;
    int wave_slots_ = 2048;  // CUs x 4 SIMDs x 2 waves: what one round of a ~240-VGPR point kernel occupies
    int device_batch_max_ = 4096;  // a device-resident prover call runs as sub-batches of at most this many blobs (ETH_KZG_AMD_DEVICE_BATCH_MAX)
    int msm_chunks_ = -1;    // -1: pick per launch (launch_msm); otherwise forced by ETH_KZG_AMD_MSM_CHUNKS
    int fused_scalars_ = -1;  // -1: k_coeffs_to_cells_scalars where enqueue_compute's conditions hold; ETH_KZG_AMD_FUSED_SCALARS=0: never, 1: at every batch size
    std::atomic<uint64_t> fused_launches_{0};  // launches of k_coeffs_to_cells_scalars so far (the parity test asks which path ran)
    bool msm_split_ = true;  // small batches: two lanes per MSM window where they still fit one round of the wave slots (ETH_KZG_AMD_MSM_SPLIT=0: off)
    hipStream_t stream_ = nullptr;
    std::recursive_mutex mu_;  // the verification / recovery / EIP-4844 / commitment paths and work_[0]: one call at a time
    static constexpr int NW = 4;  // work_[0]: the paths under mu_; work_[1..3]: compute_cells(_and_kzg_proofs) calls, concurrently
    Work work_[NW];
    std::unique_ptr<HostPool> host_pool_;
    std::once_flag host_pool_once_;

    // constants in HBM
    void* d_w8192_ = nullptr;     // Fr[8192] omega_8192^k, Montgomery
    void* d_w29_ = nullptr;       // the same in the unsaturated 9 x 29-bit form (36 B each) for the prover's Fr stages
    void* d_naf_ = nullptr;       // u32[128][2][33]: width-w NAF digits (signed bytes) of the GLV halves of omega_128^k
    Fp12w beta_;                  // cube root of unity in Fp: (beta x, y) = [lambda](x, y)
    void* d_srs_ = nullptr;       // G1Affine[4096] monomial SRS
    void* d_fk_bases_ = nullptr;  // G1Affine[128][64] FFT'd SRS vectors (batch_toeplitz.rs:46-61)
    BufferPool dev_pool_{false}, pin_pool_{true};
    void* d_tapk_ = nullptr;      // Fr29[2][2][4096]: the constants of k_coeffs_to_cells_scalars' tap for the scales 1/2 (linear-map mode) and 1/128, built from d_w29_
    Fr8 n_inv4096_, inv128_;

    // verifier / recovery constants
    void* d_coset_ = nullptr;      // Fr[8192] 7^i      (ReedSolomon coset generator, reed_solomon.rs:129)
    void* d_coset_inv_ = nullptr;  // Fr[8192] 7^-i
    Fr8 inv64_, n_inv8192_;
    std::shared_ptr<pairing::G2Prepared> g2_tau_, g2_neg_gen_;  // [tau^64]_2 and -[1]_2 (verifier.rs:88-90)
    std::shared_ptr<pairing::G2Prepared> g2_tau1_;             // [tau]_2 (EIP-4844 verification key)
    // the same three keys' prepared lines and the Frobenius constants in HBM, for k_pairing_check (the many-verifications' search for
    // wrong entries, vm_search.hpp): [tau^64]_2 | -[1]_2 | [tau]_2, 68 lines each, then the constants.  Null where a key is the point
    // at infinity (a caller's degenerate setup): such a context checks every probe on the host
    void* d_pairing_ = nullptr;
    const void* d_pairing_key(int k) const { return (const uint8_t*)d_pairing_ + (size_t)k * 68 * 192; }
    const void* d_pairing_frob() const { return d_pairing_key(3); }
    int gpu_pairing_min_ = 0;  // smallest batch of probes whose pairings run on the GPU (ETH_KZG_AMD_GPU_PAIRING_MIN); 0: never
    vm::DevicePairing device_pairing(int key) const;  // key (0, 2) next to -[1]_2 for k_pairing_check; the empty one where probes never go to the GPU

    // verify workspace: one device arena + one pinned host staging buffer, grown on demand (guarded by mu_)
    void* v_dev_ = nullptr;
    size_t v_dev_cap_ = 0;
    uint8_t* v_pin_ = nullptr;
    size_t v_pin_cap_ = 0;
    hipStream_t v_side_ = nullptr;  // verification, round 3's form: the subgroup tests run here next to the point shifts on stream_
    bool v_two_streams_ = false;    // (both chains run in ONE launch on stream_, k_pip_shift_subgroup; the two-stream form of round 3 shared hardware queues)
    hipEvent_t v_decoded_ = nullptr, v_checked_ = nullptr;
    // leaf-hashed challenge (under mu_): the leaf kernel and the read-back of its digests run on a stream of their own, behind the upload
    // (v_uploaded_) and next to the decoding kernels on stream_; v_leaves_: the digests are in the pinned slab
    hipStream_t v_leaf_stream_ = nullptr;
    hipEvent_t v_uploaded_ = nullptr, v_leaves_ = nullptr;

    // serial-path lanes (lease_serial)
    const Engine* primary_ = nullptr;   // set in an auxiliary lane
    bool auxiliary_ = false;
    std::mutex lane_busy_;              // held while a leased call runs on THIS engine
    LanePool<Engine> lanes_;            // the auxiliary lanes of a context (host_sync.hpp)
    int max_lanes_ = 4;

    // combiner of concurrent single verifications (verify_many.hip: verify_cell_kzg_proof_batch_combined)
    struct VerifyRequest;
    Combiner<VerifyRequest> combiner_{VM_SLOTS};  // at most VM_SLOTS leaders run a pass at a time (host_sync.hpp)
    std::atomic<int> verify_inflight_{0};  // single verifications on the latency path right now
    int verify_lanes_ = 1;                 // concurrent single verifications on the latency path ; the others are combined
    int comb_max_cells_ = 1024;            // larger problems always take the single path (their transcript hash is the bound)

    // many-verification path (verify_many.hip): its own lock, stream, device arena and pinned slab
    // THREE pass slots, each with its own lock, stream, device arena and pinned slab: while one pass is on the GPU the other one's
    // staging, transcript hashes and pairing checks run on the host threads (concurrent single calls are combined into passes:
    // verify_cell_kzg_proof_batch_combined lets two leaders run at a time)
    static constexpr int VM_SLOTS = 3;
    struct VmSlot {  // (its lock: vm_slots_)
        VerifyScratch vs;   // for a "pass" of ONE problem: the single path's arena on this slot's stream
        void* dev = nullptr;
        size_t dev_cap = 0;
        uint8_t* pin = nullptr;
        size_t pin_cap = 0;
        // flat device source: the pinned mirror of the commitments and indices of the call's problems (those within the size bound, back
        // to back); `ordered` puts the caller's stream in front of the pass's
        uint8_t* src_pin = nullptr;
        size_t src_pin_cap = 0;
        hipEvent_t ordered = nullptr;
        // what the host threads hash is in the pinned slab: the leaf digests (leaf-hashed challenges), or the proofs and cells the flat
        // device source brings down for the reference's transcript
        hipEvent_t hash_inputs_down = nullptr;
    };
    VmSlot vm_slot_[VM_SLOTS];
    SlotSet<VM_SLOTS> vm_slots_;  // leases of the pass slots (host_sync.hpp)
    // a pass slot taken for one pass (verify_many.hip): the slot, its lock, and the stream the slot runs on
    struct PassSlot {
        VmSlot* slot;
        std::unique_lock<std::mutex> lock;
        hipStream_t stream;
    };
    PassSlot lease_pass_slot(bool prefer_idle_work_set);
    struct PointPass;  // one pass of verify_kzg_proof_many on such a slot (point_many.hip)
    struct CellManyPass;  // one pass of verify_cell_kzg_proof_batch_many on such a slot (verify_many.hip)
    // the column source's once-per-call work; the body every source shares: the call cut into concurrent parts
    int verify_data_columns_many(int B, const VerifyManyInput& in, int* verified, int* status, VerifyManyTap* tap);
    int verify_cell_kzg_proof_batch_many_parts(int B, const VerifyManyInput& in, int* verified, int* status, VerifyManyTap* tap);
    // the part of a many-verification call that runs as passes of its own on one slot: the whole call, or one of its concurrent parts
    int verify_cell_kzg_proof_batch_many_part(int B, const VerifyManyInput& in, int* verified, int* status, VerifyManyTap* tap);
    std::unique_ptr<HostPool> stage_pool_;  // staging of single verifications (a few threads: the lane + the pass slots run side by side)
    std::once_flag stage_pool_once_;
    std::unique_ptr<HostPool> vm_pool_;  // the host threads of the many-verification passes (hashes, staging, pairing checks)
    std::once_flag vm_pool_once_;
    struct VmHost {
        int T;           // threads a pass spreads its host work over, the caller's among them
        HostPool* pool;  // the T - 1 others (made on first use)
    };
    VmHost vm_host();
    bool vm_search_ = true;  // ETH_KZG_AMD_VM_SEARCH=0: a pass whose folded check fails is re-checked problem by problem (round 3's form)
    int vm_small_max_ = -1;  // passes of at most this many problems take the short-chain form (verify_many.hip); -1: 2 x host threads
    uint8_t* vd_pin_ = nullptr;  // device-resident verification: the host mirror the transcript hash reads (grow-only, guarded by mu_)
    size_t vd_pin_cap_ = 0;
    static constexpr int VD_CHUNKS = 8;
    hipEvent_t vd_events_[VD_CHUNKS] = {};

    // small-batch circulant form of the two G1 transforms: term list, doubling tables (allocated on first use)
    void *d_circ_terms_ = nullptr;
    // verification batches of at least this many cells build byte-shifted point copies before the challenge is known
    // (k_verify.hip: k_pip_shift): behind the transcript hash for large batches, next to the subgroup tests (second stream) for
    // small ones.  ETH_KZG_AMD_PIP_SHIFT_MIN raises it (tests: the windowed form as the cross-check)
    int pip_shift_min_ = 1;
    int circ_T_ = 0, circ_per_lane_ = 0, circ_max_ = 2;  // largest batch on the circulant form: the measured cross-over with the compiled linear map (engine.hip: the constructor)
    Fr8 seg_shift_[3];  // 2^32, 2^64, 2^96 in Montgomery form
    // the two G1 transforms as one compiled linear map (g1_linmap.hpp, k_g1slp.hip).  SEVERAL compilations of the same map:
    // the throughput optimum (fewest point operations: 350 constant multiplications, 8-way Toom-Cook) for batches that fill
    // the chip, and depth-optimised ones for batches that do not -- there a dependency level lasts as long as its longest
    // operation and a constant multiplication has a SIMD to itself as long as waves <= SIMDs, so more multiplications with
    // shallower, doubling-free evaluation / interpolation trees (Karatsuba: 712 multiplications, 13 levels of single
    // additions instead of 25 levels with runs of up to 7 doublings) are faster.  Picked per launch by the number of 64-blob
    // lane groups (pick_slp_program); built on first use except the two tuned schedules.
    struct SlpLaunch { int kind, first, count; };
    enum SlpProgramId { SLP_TUNED_FUSED = 0, SLP_TUNED = 1, SLP_KARATSUBA = 2, SLP_DEPTH_456 = 3, SLP_DEPTH_606 = 4, SLP_DEPTH_372 = 5, SLP_COUNT = 6 };
    struct SlpProgram {
        std::vector<SlpLaunch> launches;
        void *d_words = nullptr, *d_naf = nullptr;  // d_naf may be shared with another program of the same plan (owns_naf)
        bool owns_naf = false, ready = false;
        int n_slots = 0;
        size_t n_words = 0;          // words behind d_words (4 per operation)
        std::vector<Fr8> consts;     // the constants d_naf was recoded from, Montgomery form
        int info[4] = {0, 0, 0, 0};  // constant multiplications, additions, doublings, launches
    };
    SlpProgram slp_prog_[SLP_COUNT];
    std::mutex slp_build_mu_;
    std::vector<Fr8> w128_;                       // omega_128^e, kept for the programs built on first use
    const SlpProgram& slp_program(int id);        // builds it if need be (engine.hip: build_slp_program)
    void build_slp_program(int id);
    int pick_slp_program(int lanes) const;        // lanes = blobs rounded up to 64
    int slp_force_ = -1;                          // ETH_KZG_AMD_SLP_PROGRAM: this program at every batch size (tests, A/B runs)
    // a phase = one multiplication launch (level0 < 0) or a run of cheap dependency levels executed by ONE ticket-walking launch
    int slp_fuse_min_ = 1024;  // measured: 512 blobs 5.47 (plain) against 5.55 ms (fused), 2048 blobs 16.13 against 15.93 ms
    int slp_info_[4] = {0, 0, 0, 0};  // constant multiplications, additions, doublings, launches of the tuned program
    Fr8 half_;  // 1/2 in Montgomery form: the scaling folded into the MSM scalars in linear-map mode

    // work_[0] under its historical names (grown on demand, guarded by mu_)
    int& cap_ = work_[0].cap;
    void *&d_coeffs_ = work_[0].coeffs, *&d_canon_ = work_[0].canon, *&d_scalars_ = work_[0].scalars, *&d_X_ = work_[0].X;
    int*& d_status_ = work_[0].status;
    uint8_t *d_in_ = nullptr, *d_cells_ = nullptr, *d_proofs_ = nullptr;  // staging for host API
    int stage_cap_ = 0;
};

}  // namespace kzg
