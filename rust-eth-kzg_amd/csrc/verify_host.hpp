// The host's share of verification and recovery that is pure computation over bytes: input validation, de-duplication, the scalar
// codecs and the Fiat-Shamir transcripts (the reference's four, the leaf-hashed challenge of the cell verifier and the leaves, seed and
// weights of the point many-verification), each stated ONCE for verify.hip, verify_many.hip, point_many.hip, eip4844.hip and recover.hip.
// No HIP call in here, everything inline: tests/c/test_verify_host.cpp, test_leaf_transcript.cpp, test_many_leaf.cpp,
// test_point_many.cpp, test_blob_many.cpp, test_data_columns.cpp, test_partial_columns.cpp and test_blob_cells.cpp run it on the CPU
// against hashlib.
// Reference: crates/eip7594/src/verifier.rs:49-164, crates/cryptography/kzg_multi_open/src/fk20/verifier.rs:269-328,
// crates/eip4844/src/verifier.rs:155-262, crates/eip7594/src/recovery.rs:90-146, crates/cryptography/bls12_381/src/lib.rs:128-140.
#pragma once
#include "field.hpp"
#include "sha256.hpp"

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace kzg {

// the geometry of a blob on the host side (the kernels' copy: kcommon.hpp)
constexpr int N_BLOB = 4096, N_EXT = 8192, N_CELLS = 128, CELL_LEN = 64, BYTES_PER_BLOB = 131072, BYTES_PER_CELL = 2048;
// what the validations return: Status OK / ERR_INPUT and the bound MAX_CELLS_PER_VERIFICATION of engine.hpp (verify.hip asserts the three)
constexpr int INPUT_VALID = 0, INPUT_INVALID = 3;
constexpr uint64_t INPUT_MAX_CELLS = (1u << 24) - 1;

inline void be64(uint64_t v, uint8_t* o) { for (int b = 0; b < 8; b++) o[b] = (uint8_t)(v >> (56 - 8 * b)); }
inline int brp7(int v) { int r = 0; for (int i = 0; i < 7; i++) r |= ((v >> i) & 1) << (6 - i); return r; }

// ---- scalars: 32 big-endian bytes <-> Fr
inline Fr fr_words_from_be(const uint8_t* b) {  // the integer as it stands: neither reduced nor Montgomery
    Fr x;
    for (int i = 0; i < 8; i++)
        x.v[7 - i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
    return x;
}
// reduce_bytes_to_scalar_bias (crates/cryptography/bls12_381/src/lib.rs:128-140): 256-bit big-endian integer mod r, Montgomery
inline Fr fr_from_digest(const uint8_t* b) {
    Fr x = fr_words_from_be(b);
    while (geq_mod<FrParams>(x.v)) {  // 2^256 < 3r: at most two subtractions
        uint32_t t[8];
        sub_limbs<8>(t, x.v, FrParams::MOD);
        memcpy(x.v, t, 32);
    }
    return to_mont(x);
}
inline bool fr_from_be_canonical(Fr& out_mont, const uint8_t* b) {  // deserialize_bytes_to_scalar (serialization/src/lib.rs:50-63)
    const Fr x = fr_words_from_be(b);
    if (geq_mod<FrParams>(x.v)) return false;
    out_mont = to_mont(x);
    return true;
}
inline void fr_to_be(uint8_t* o, const Fr& canon) {
    for (int i = 0; i < 8; i++) {
        uint32_t w = canon.v[7 - i];
        o[4 * i] = (uint8_t)(w >> 24); o[4 * i + 1] = (uint8_t)(w >> 16); o[4 * i + 2] = (uint8_t)(w >> 8); o[4 * i + 3] = (uint8_t)w;
    }
}

// ---- the cell verifier's inputs
// validation (verifier.rs:123-164), before anything is sized by a count or read through a pointer array
inline int validate_cell_batch(uint64_t n_commitments, uint64_t n_indices, uint64_t n_cells, uint64_t n_proofs, const uint64_t* cell_indices) {
    if (!(n_commitments == n_indices && n_commitments == n_cells && n_commitments == n_proofs)) return INPUT_INVALID;
    if (n_cells > INPUT_MAX_CELLS) return INPUT_INVALID;  // (engine.hpp: the 24-entry power table, 32-bit positions)
    for (uint64_t i = 0; i < n_indices; i++)
        if (cell_indices[i] >= (uint64_t)N_CELLS) return INPUT_INVALID;
    return INPUT_VALID;
}
// deduplicate_with_indices (verifier.rs:49-65): byte equality, first-occurrence order -> the unique commitments, the row of every entry.
// at(i) = the 48 bytes of entry i: a pointer list, or flat bytes (the device-resident many-verification's mirror)
template <class At>
inline void dedup_commitments_at(uint64_t n, At at, std::vector<const uint8_t*>& uniq, std::vector<int>& row) {
    uniq.clear();
    row.resize(n);
    std::map<std::string, int> seen;
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t* c = at(i);
        std::string key((const char*)c, 48);
        auto it = seen.find(key);
        if (it == seen.end()) { it = seen.emplace(key, (int)uniq.size()).first; uniq.push_back(c); }
        row[i] = it->second;
    }
}
inline void dedup_commitments(uint64_t n, const uint8_t* const* commitments, std::vector<const uint8_t*>& uniq, std::vector<int>& row) {
    dedup_commitments_at(n, [commitments](uint64_t i) { return commitments[i]; }, uniq, row);
}
inline void dedup_commitments_flat(uint64_t n, const uint8_t* flat48, std::vector<const uint8_t*>& uniq, std::vector<int>& row) {
    dedup_commitments_at(n, [flat48](uint64_t i) { return flat48 + i * 48; }, uniq, row);
}
// cell_starts of the device-resident many-verification (c_eth_kzg.h): n_batches + 1 entries, the first 0, non-decreasing; problem b is
// the entries [cell_starts[b], cell_starts[b + 1]) of the flat arrays.  How long a problem may be is the problem's own validation
// (validate_cell_batch: status 3 for that problem), not the array's.
inline int validate_cell_starts(uint64_t n_batches, const uint64_t* cell_starts) {
    if (n_batches == 0) return INPUT_VALID;
    if (!cell_starts || cell_starts[0] != 0) return INPUT_INVALID;
    for (uint64_t b = 0; b < n_batches; b++)
        if (cell_starts[b + 1] < cell_starts[b]) return INPUT_INVALID;
    return INPUT_VALID;
}
// ---- eth_kzg_amd_verify_data_columns / _device (c_eth_kzg.h): the columns of one block over ONE commitment list.  Column j is the
// problem (commitments as given, n_blobs copies of column_indices[j], cells[j], proofs[j]) of the many-verification; there is no new
// transcript.  What the call refuses as a whole, before the context is touched:
constexpr uint64_t DATA_COLUMNS_MAX = 1u << 24;
inline int validate_data_columns_call(uint32_t flags, uint32_t known_flags, uint64_t n_blobs, uint64_t n_columns, bool commitments_null,
                                      bool indices_null, bool cells_null, bool proofs_null, bool verified_null) {
    if (flags & ~known_flags) return INPUT_INVALID;
    if (n_columns > DATA_COLUMNS_MAX) return INPUT_INVALID;
    if (n_columns == 0) return INPUT_VALID;
    if (verified_null || indices_null) return INPUT_INVALID;
    // (a NULL array with a non-zero count, also when the count is beyond the bound and every column will be status 3 unread)
    if (n_blobs != 0 && (commitments_null || cells_null || proofs_null)) return INPUT_INVALID;
    return INPUT_VALID;
}
// the status of one column at validation: validate_cell_batch of the expanded problem (four equal lengths, n_blobs copies of the index;
// an empty problem is valid without its index being read)
inline int validate_data_column(uint64_t n_blobs, uint64_t column_index) {
    if (n_blobs > INPUT_MAX_CELLS) return INPUT_INVALID;
    if (n_blobs != 0 && column_index >= (uint64_t)N_CELLS) return INPUT_INVALID;
    return INPUT_VALID;
}
// The block's commitments de-duplicated ONCE per call: every column's expanded problem has this same unique list and these same rows
// (dedup_commitments of n_blobs entries does not look at the column), so every column's transcript and ROOT see exactly it.
struct ColumnCommitments {
    std::vector<uint8_t> own;          // (device form) the 48 n_blobs bytes as they came down
    std::vector<const uint8_t*> uniq;  // first-occurrence order
    std::vector<int> row;              // per blob: index into uniq
    void from_list(uint64_t n_blobs, const uint8_t* const* commitments) { dedup_commitments(n_blobs, commitments, uniq, row); }
    void from_own(uint64_t n_blobs) { dedup_commitments_flat(n_blobs, own.data(), uniq, row); }
};

// ---- eth_kzg_amd_verify_partial_data_columns / _device (c_eth_kzg.h): columns that carry a BITMAP of the blobs present and cells and
// proofs for those blobs only (the partial data column sidecar of cell-level dissemination).  present[j]: W = ceil(n_blobs / 64) words,
// bit i % 64 of word i / 64 = blob i (the convention of present_masks in eth_kzg_amd_recover_cells_and_proofs_device).  Column j is the
// problem (commitments[i] for its set bits i in ascending order, m_j copies of column_indices[j], cells[j], proofs[j]) of the
// many-verification; there is no new transcript.  A fifth spelling of the column source, not a new verifier.
inline uint64_t partial_words(uint64_t n_blobs) { return (n_blobs + 63) / 64; }
// what the call refuses as a whole, before the context is touched
inline int validate_partial_columns_call(uint32_t flags, uint32_t known_flags, uint64_t n_blobs, uint64_t n_columns, bool commitments_null,
                                         bool indices_null, bool present_null, bool cells_null, bool proofs_null, bool verified_null) {
    if (flags & ~known_flags) return INPUT_INVALID;
    if (n_columns > DATA_COLUMNS_MAX) return INPUT_INVALID;
    if (n_columns == 0) return INPUT_VALID;
    if (verified_null || indices_null) return INPUT_INVALID;
    if (n_blobs != 0 && (present_null || commitments_null || cells_null || proofs_null)) return INPUT_INVALID;
    return INPUT_VALID;
}
inline uint64_t popcount64(uint64_t w) { uint64_t c = 0; for (; w; w &= w - 1) c++; return c; }
// The entries a column occupies in the packed device arrays: the set bits of ALL its W words, stray bits included, so that a refused
// column is skipped without being read.
inline uint64_t partial_column_entries(uint64_t n_blobs, const uint64_t* words) {
    uint64_t c = 0;
    for (uint64_t w = 0; w < partial_words(n_blobs); w++) c += popcount64(words[w]);
    return c;
}
// THE STRAY-BIT RULE and the status of one column at validation: 3 for a set bit at or beyond n_blobs (only the last word can hold
// one) or, where the column holds a cell, an index >= 128 (validate_cell_batch of the expanded problem: an empty problem is valid
// without its index being read).  n_blobs beyond the bound: every column, nothing read.  *count = m_j, the set bits below n_blobs.
inline int validate_partial_column(uint64_t n_blobs, uint64_t column_index, const uint64_t* words, uint64_t* count) {
    *count = 0;
    if (n_blobs > INPUT_MAX_CELLS) return INPUT_INVALID;
    const uint64_t W = partial_words(n_blobs);
    if (n_blobs % 64 != 0 && (words[W - 1] >> (n_blobs % 64)) != 0) return INPUT_INVALID;
    uint64_t m = 0;
    for (uint64_t w = 0; w < W; w++) m += popcount64(words[w]);
    if (m != 0 && column_index >= (uint64_t)N_CELLS) return INPUT_INVALID;
    *count = m;
    return INPUT_VALID;
}
// The columns of a call, made ONCE (c_api.cpp, before the call is cut over a device list): per column its status at validation, m_j
// (0 for a refused column), its first entry in the packed device arrays (start, n_columns + 1 entries: a refused column keeps its
// place there) and the blobs it holds in ascending order (blob[blob_start[j] .. blob_start[j + 1]); nothing for a refused column).
// words_of(j) -> the W words of column j (a pointer list, or the flat array of the device form).
struct PartialColumns {
    uint64_t n_blobs = 0, W = 0;
    std::vector<int> status;
    std::vector<uint64_t> count, start, blob_start;
    std::vector<uint32_t> blob;
    template <class WordsOf>
    void build(uint64_t n_blobs_, uint64_t n_columns, const uint64_t* column_indices, WordsOf words_of) {
        n_blobs = n_blobs_; W = partial_words(n_blobs);
        const bool unread = n_blobs > INPUT_MAX_CELLS;  // nothing of the bitmaps is read
        status.assign(n_columns, INPUT_INVALID); count.assign(n_columns, 0); start.assign(n_columns + 1, 0); blob_start.assign(n_columns + 1, 0);
        blob.clear();
        for (uint64_t j = 0; j < n_columns; j++) {
            const uint64_t* const words = unread || W == 0 ? nullptr : words_of(j);
            if (!unread) status[j] = validate_partial_column(n_blobs, column_indices[j], words, &count[j]);
            start[j + 1] = start[j] + (unread || W == 0 ? 0 : partial_column_entries(n_blobs, words));
            if (status[j] == INPUT_VALID)
                for (uint64_t w = 0; w < W; w++)
                    for (uint64_t bits = words[w]; bits; bits &= bits - 1) blob.push_back((uint32_t)(w * 64 + (uint64_t)__builtin_ctzll(bits)));
            blob_start[j + 1] = blob.size();
        }
    }
    void from_list(uint64_t n_blobs_, uint64_t n_columns, const uint64_t* column_indices, const uint64_t* const* present) {
        build(n_blobs_, n_columns, column_indices, [present](uint64_t j) { return present[j]; });
    }
    void from_flat(uint64_t n_blobs_, uint64_t n_columns, const uint64_t* column_indices, const uint64_t* present) {
        const uint64_t w = partial_words(n_blobs_);
        build(n_blobs_, n_columns, column_indices, [present, w](uint64_t j) { return present + j * w; });
    }
    uint64_t total_cells() const { return blob.size(); }
};
// What differs per column, stated once.  (1) THE TRANSCRIPT'S ROWS.  The expanded problem is de-duplicated alone
// (dedup_commitments over the commitments of its present blobs): its unique list holds the call's unique commitments that its present
// blobs refer to, in the order in which the column's OWN blobs first name them -- with repeated commitments that need not be the order
// of the call's list (blobs X Y X with blobs 1 and 2 present: Y X) -- and its rows are ranks inside that list.  Under flags = 0 the
// reference transcript carries that list, its length and those rows (uniq, row); the kernels go on reading the pass-wide row of every
// cell (pass_row).  (2) THE PAIR LIST.  The column's (column, commitment) pairs are that same list as indices into the call's unique
// list (pair_u): one weight and one product each, never more than the column has cells.
struct PartialColumnView {
    std::vector<const uint8_t*> uniq;  // the column's own unique list
    std::vector<int> row;              // per cell: rank in uniq
    std::vector<int> pass_row;         // per cell: index into the call's unique list
    std::vector<int> pair_u;           // per entry of uniq: its index in the call's unique list
};
inline void partial_column_view(const ColumnCommitments& cc, const uint32_t* blobs, uint64_t m, PartialColumnView& v) {
    v.uniq.clear(); v.pair_u.clear();
    v.row.resize(m); v.pass_row.resize(m);
    std::map<int, int> rank;  // call-wide row -> rank in the column's list
    for (uint64_t k = 0; k < m; k++) {
        const int u = cc.row[blobs[k]];
        auto it = rank.find(u);
        if (it == rank.end()) { it = rank.emplace(u, (int)v.uniq.size()).first; v.uniq.push_back(cc.uniq[(size_t)u]); v.pair_u.push_back(u); }
        v.row[k] = it->second;
        v.pass_row[k] = u;
    }
}
// The columns of a partial call that go on: kept column k is the caller's column keep[k].
inline std::vector<uint64_t> vm_kept_partial_columns(const PartialColumns& pc, uint64_t base, uint64_t n_columns) {
    std::vector<uint64_t> keep;
    for (uint64_t b = 0; b < n_columns; b++)
        if (pc.status[base + b] == INPUT_VALID) keep.push_back(b);
    return keep;
}

// validate_recovery_inputs (recovery.rs:90-146)
inline int validate_recovery(uint64_t n_cells, uint64_t n_indices, const uint64_t* cell_indices) {
    if (n_indices != n_cells) return INPUT_INVALID;
    for (uint64_t i = 0; i < n_indices; i++)
        if (cell_indices[i] >= (uint64_t)N_CELLS) return INPUT_INVALID;
    for (uint64_t i = 1; i < n_indices; i++)
        if (!(cell_indices[i - 1] < cell_indices[i])) return INPUT_INVALID;
    if (n_indices < (uint64_t)N_CELLS / 2 || n_indices > (uint64_t)N_CELLS) return INPUT_INVALID;
    return INPUT_VALID;
}
// The status of the index list of a column recovery (eth_kzg_amd_recover_data_columns and its checked form): validate_recovery of the
// per-blob list every blob of the call expands into (the count first: a list of more than 128 entries is refused unread).
inline int column_list_status(uint64_t n_columns, const uint64_t* column_indices) {
    if (n_columns < (uint64_t)N_CELLS / 2 || n_columns > (uint64_t)N_CELLS || !column_indices) return INPUT_INVALID;
    return validate_recovery(n_columns, n_columns, column_indices);
}

// ---- compute_fiat_shamir_challenge of the cell verifier (fk20/verifier.rs:269-328), cell by cell: valid inputs are canonical
// encodings, so the transcript is the input bytes themselves.  It always covers the WHOLE batch (n_all cells, m unique commitments).
class CellBatchTranscript {
public:
    CellBatchTranscript(int m, int n_all, const uint8_t* const* uniq) {
        uint8_t hdr[16 + 32];
        memcpy(hdr, "RCKZGCBATCH__V1_", 16);
        be64(N_BLOB, hdr + 16); be64(CELL_LEN, hdr + 24); be64((uint64_t)m, hdr + 32); be64((uint64_t)n_all, hdr + 40);
        sh_.update(hdr, sizeof hdr);
        for (int i = 0; i < m; i++) sh_.update(uniq[i], 48);
    }
    void absorb(int row, uint64_t index, const uint8_t* cell, const uint8_t* proof) {
        uint8_t ix[16];
        be64((uint64_t)row, ix); be64(index, ix + 8);
        sh_.update(ix, 16);
        sh_.update(cell, BYTES_PER_CELL);
        sh_.update(proof, 48);
    }
    Fr finish() {  // the challenge r, Montgomery
        sh_.finish(digest_);
        return fr_from_digest(digest_);
    }
    const uint8_t* digest() const { return digest_; }  // after finish(): the 32 bytes r was reduced from
private:
    Sha256 sh_;
    uint8_t digest_[32];
};

// ---- the leaf-hashed challenge of the cell verifier (ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT; the reference has nothing like it).
// The transcript above is ONE SHA-256 over every byte of the batch: serial by construction, 7.2 ms of a host core for 8192 cells.
// Only the verdict crosses the ABI, never r, so a challenge that binds the same bytes through a two-level hash serves as well:
//   LEAF_k = SHA-256("RCKZGCBATCHLEAF1" | be64(k) | be64(cell_indices[k]) | commitments[k] | proofs[k] | cells[k])      2176 bytes
//   ROOT   = SHA-256("RCKZGCBATCHROOT1" | be64(4096) | be64(64) | be64(n) | LEAF_0 | .. | LEAF_{n-1})
//   r      = fr_from_digest(ROOT)
// k is the position in the caller's list and commitments[k] the caller's 48 bytes of entry k (no de-duplication).  A leaf is 34
// blocks: the header is exactly two, every 64-byte row of the cell is one, and the 35th compression is constant padding (0x80,
// zeroes, the bit length 17408).  The leaves are independent, one lane each on the GPU (k_sha256.hip: k_sha256_cell_leaves); this
// class is the host's statement of them and of the root, which the host hashes from the n x 32 digest bytes that come down.
// Soundness.  r is a hash of every input byte: the leaves bind the contents, the root binds their order and number, and two
// batches with one r are a SHA-256 collision (in a leaf, or in the root).  The batch equation is the reference's: a batch that
// holds a wrong proof passes only if r is a root of a non-zero polynomial of degree below n over Fr -- the argument of the
// reference's own challenge, which asks of the hash nothing else.  Valid batches verify under any r, and whether a call is Err or
// Ok(false) is decided by validation and decoding, before r is used.
// The many-verification (verify_many.hip; eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex / _many_device_ex with the flag) takes, for
// every problem of a call, exactly this challenge of the problem alone: k restarts at 0 in each problem, ROOT carries the problem's own
// n (cell_leaf_root below).  Its folding weights (fold_seed, fold_weight) then hash the problems' ROOTs where they hash the reference
// transcript's digests otherwise: every ROOT is a hash of every input byte of its problem, so the weights still hang on every input
// byte of the pass and cannot be predicted before all of them are fixed -- the argument of the fold is unchanged.
// Out of scope: _partial / _combine and the combiner of concurrent single calls keep the reference's transcript; no environment knob
// moves an unflagged symbol onto this one; the Node binding does not pass the flag.
class CellLeafTranscript {
public:
    static constexpr size_t LEAF_BYTES = 16 + 8 + 8 + 48 + 48 + BYTES_PER_CELL;  // 2176 = 34 blocks
    static void leaf(uint64_t k, uint64_t index, const uint8_t* commitment, const uint8_t* proof, const uint8_t* cell, uint8_t out[32]) {
        uint8_t hdr[128];
        memcpy(hdr, "RCKZGCBATCHLEAF1", 16);
        be64(k, hdr + 16); be64(index, hdr + 24);
        memcpy(hdr + 32, commitment, 48);
        memcpy(hdr + 80, proof, 48);
        Sha256 sh;
        sh.update(hdr, sizeof hdr);
        sh.update(cell, BYTES_PER_CELL);
        sh.finish(out);
    }
    // leaves: the n digests in the caller's order, 32 bytes each -> the challenge r, Montgomery
    Fr root(uint64_t n, const uint8_t* leaves) {
        uint8_t hdr[16 + 24];
        memcpy(hdr, "RCKZGCBATCHROOT1", 16);
        be64(N_BLOB, hdr + 16); be64(CELL_LEN, hdr + 24); be64(n, hdr + 32);
        Sha256 sh;
        sh.update(hdr, sizeof hdr);
        sh.update(leaves, (size_t)n * 32);
        sh.finish(digest_);
        return fr_from_digest(digest_);
    }
    const uint8_t* digest() const { return digest_; }  // after root(): the 32 bytes r was reduced from
private:
    uint8_t digest_[32];
};
static_assert(CellLeafTranscript::LEAF_BYTES == 34 * 64, "the header is two blocks and the cell thirty-two");
// the challenge of problem b of a many-verification pass: leaves = the digests of the pass's cells back to back, 32 bytes each, entry 0
// the cell starts[0]; problem b holds the cells [starts[b], starts[b + 1]).  digest_out: the problem's ROOT.
template <class Int>
inline Fr cell_leaf_root(const uint8_t* leaves, const Int* starts, size_t b, uint8_t digest_out[32]) {
    CellLeafTranscript t;
    const Fr r = t.root((uint64_t)(starts[b + 1] - starts[b]), leaves + (size_t)(starts[b] - starts[0]) * 32);
    memcpy(digest_out, t.digest(), 32);
    return r;
}

// ---- compute_fiat_shamir_challenge of EIP-4844 (eip4844/src/verifier.rs:155-196): H(header | blob | commitment) mod r
inline void blob_challenge_header(uint8_t hdr[32]) {
    memcpy(hdr, "FSBLOBVERIFY_V1_", 16);
    memset(hdr + 16, 0, 16);
    hdr[16 + 14] = 0x10;  // u128 big-endian 4096
}
inline Fr blob_challenge(const uint8_t* blob, const uint8_t* commitment) {
    Sha256 sh;
    uint8_t hdr[32], dig[32];
    blob_challenge_header(hdr);
    sh.update(hdr, 32);
    sh.update(blob, BYTES_PER_BLOB);
    sh.update(commitment, 48);
    sh.finish(dig);
    return fr_from_digest(dig);
}
// compute_r_powers_for_verify_kzg_proof_batch (eip4844/src/verifier.rs:201-262) -> r, Montgomery; z_i Montgomery, y_i canonical
inline Fr blob_batch_weight(int n, const uint8_t* const* commitments, const Fr* z_mont, const Fr* y_canon, const uint8_t* const* proofs) {
    Sha256 sh;
    uint8_t hdr[32];
    memcpy(hdr, "RCKZGBATCH___V1_", 16);
    be64(N_BLOB, hdr + 16); be64((uint64_t)n, hdr + 24);
    sh.update(hdr, 32);
    for (int i = 0; i < n; i++) {
        uint8_t zy[64];
        fr_to_be(zy, from_mont(z_mont[i]));
        fr_to_be(zy + 32, y_canon[i]);
        sh.update(commitments[i], 48);
        sh.update(zy, 64);
        sh.update(proofs[i], 48);
    }
    uint8_t dig[32];
    sh.finish(dig);
    return fr_from_digest(dig);
}

// ---- folding weights of a many-verification pass: rho_i = SHA-256(seed | i) truncated to 127 bits, seed = SHA-256 over ALL the
// challenges' digests of the pass (so no weight can be predicted before every input byte is fixed)
inline void fold_seed(const uint8_t* digests, size_t bytes, uint8_t seed[32]) {
    Sha256 sh;
    sh.update((const uint8_t*)"RCKZGCBATCHFOLD1", 16);
    sh.update(digests, bytes);
    sh.finish(seed);
}
inline void fold_weight(const uint8_t seed[32], uint64_t i, uint32_t out4[4]) {
    Sha256 sh;
    uint8_t ix[8], dg[32];
    be64(i, ix);
    sh.update(seed, 32);
    sh.update(ix, 8);
    sh.finish(dg);
    memcpy(out4, dg, 16);
    out4[3] &= 0x7fffffffu;
    if ((out4[0] | out4[1] | out4[2] | out4[3]) == 0) out4[0] = 1;  // a weight of zero would drop its problem from the check
}

// ---- the bookkeeping of the cell many-verification (verify_many.hip; tests/c/test_vm_plan.cpp): integers in, a vector out, no HIP.
// The PARTS of a call of B problems, cells_of(b) cells each: cut points 0 = c_0 < .. < c_P = B (B = 0: {0}).  A call below min_problems
// problems or min_cells cells is one part; a larger one is cut into at most max_parts equal shares of its cells: behind the problem
// with which the running total reaches the next share, never behind the last problem.
template <class CellsOf>
inline std::vector<int> vm_call_parts(int B, CellsOf cells_of, int min_problems, uint64_t min_cells, int max_parts) {
    std::vector<int> cut{0};
    if (B == 0) return cut;
    uint64_t total = 0, acc = 0;
    for (int b = 0; b < B && max_parts > 1 && B >= min_problems; b++) total += cells_of(b);
    for (int b = 0; b < B && total >= min_cells; b++) {
        acc += cells_of(b);
        if ((int)cut.size() < max_parts && acc * max_parts >= total * cut.size() && b + 1 < B) cut.push_back(b + 1);
    }
    cut.push_back(B);
    return cut;
}
// The CHUNK that begins at problem b0 ends in front of the problem returned: as many as hold at most chunk_cells cells, and at least one.
template <class CellsOf>
inline int vm_chunk_end(int B, int b0, CellsOf cells_of, uint64_t chunk_cells) {
    int b1 = b0;
    uint64_t n = 0;
    while (b1 < B && (b1 == b0 || n + cells_of(b1) <= chunk_cells)) n += cells_of(b1++);
    return b1;
}
// The COPIES that bring the problems that take part, in order, back to back to a destination: one run per stretch of them that
// follow each other in the source.  (A problem that takes no part and holds entries ends a run: the source goes on behind them.)
struct CopyRun { uint64_t src, len, dst; };
template <class SrcOf, class LenOf, class Takes>
inline std::vector<CopyRun> vm_copy_runs(int B, SrcOf src_of, LenOf len_of, Takes takes) {
    std::vector<CopyRun> runs;
    uint64_t at = 0;
    for (int b = 0; b < B; b++) {
        const uint64_t len = takes(b) ? (uint64_t)len_of(b) : 0;
        if (!len) continue;
        if (!runs.empty() && runs.back().src + runs.back().len == (uint64_t)src_of(b)) runs.back().len += len;
        else runs.push_back({(uint64_t)src_of(b), len, at});
        at += len;
    }
    return runs;
}
// The columns of a column call that go on (validate_data_column accepts them): kept column k is the caller's column keep[k].
inline std::vector<uint64_t> vm_kept_columns(uint64_t n_blobs, uint64_t n_columns, const uint64_t* column_indices) {
    std::vector<uint64_t> keep;
    for (uint64_t b = 0; b < n_columns; b++)
        if (validate_data_column(n_blobs, column_indices[b]) == INPUT_VALID) keep.push_back(b);
    return keep;
}

// ---- eth_kzg_amd_verify_kzg_proof_many / _many_device (point_many.hip): MANY items (commitment, z, y, proof), a verdict for each --
// exactly what Verifier::verify_kzg_proof (crates/eip4844/src/verifier.rs:19-44) says of the item alone.  The reference has nothing
// like it.  Item equation, as the single call evaluates it (eip4844.hip: verify_kzg_proof_host):
//     e(pi_i, [tau]_2) e(C_i + z_i pi_i - y_i G, -[1]_2) = 1
// A call is cut into passes of at most POINT_MANY_PASS items, in the caller's order (point_pass_end).  Within a pass of n_p items:
//   LEAF_i = SHA-256("RCKZGPROOFLEAF_1" | commitment_i | z_i | y_i | proof_i)           the caller's 160 bytes behind the domain
//   SEED   = SHA-256("RCKZGPROOFFOLD_1" | be64(n_p) | LEAF_0 | .. | LEAF_{n_p - 1})
//   rho_i  = fold_weight(SEED, i)                                                      127 bits, never zero; i = position in the pass
// An item refused at validation (point_item_status != 0) is hashed like any other and takes no part in any sum.  The pair of a range R:
//     ( sum_{i in R, status 0} rho_i pi_i ,  sum_{i in R, status 0} rho_i (C_i + z_i pi_i - y_i G) )
// Soundness.  SEED is a hash of every input byte of the pass: the leaves bind the contents of the items, SEED binds their order and
// number, and two passes with one SEED are a SHA-256 collision (in a leaf, or in the seed).  So no weight can be predicted before every
// byte of every item is fixed.  Write E_i for the item's own pairing value e(pi_i, [tau]_2) e(C_i + z_i pi_i - y_i G, -[1]_2), an
// element of the pairing group of prime order r; the pair of R passes the check iff prod_{i in R} E_i^(rho_i) = 1.  If every item of
// R is valid that holds for any weights.  If some E_j != 1, then for fixed other weights at most one residue of rho_j mod r makes the
// product 1, and rho_j is one of 2^127 - 1 values the prover could not choose: a range that holds a wrong item passes with probability
// 2^-127 (the argument of the cell verifier's fold above, and of the powers of r in the reference's own batch check,
// kzg_single_open/src/verifier.rs:76-107).  A pass whose full-range pair passes therefore holds valid items only; otherwise the wrong
// items are SEARCHED by checking the pairs of sub-ranges down to single items, and a single item whose pair fails is wrong EXACTLY:
// E_i^(rho_i) != 1 with 0 < rho_i < r means E_i != 1.  Whether an item's status is 0, 1 or 2 is decided before any weight is used.
// The host form hashes the leaves on the host threads, the device form on the GPU (k_point_many.hip: k_pm_leaf_bodies + k_sha256_many);
// both compute the same leaves, seed and weights.
constexpr uint64_t POINT_MANY_MAX_ITEMS = 1u << 24;
constexpr int POINT_MANY_PASS = 16384;  // the product's P; not part of the contract
struct PointProofTranscript {
    static constexpr size_t LEAF_BYTES = 16 + 48 + 32 + 32 + 48;  // 176: two blocks and 48 bytes
    static void leaf(const uint8_t* commitment, const uint8_t* z, const uint8_t* y, const uint8_t* proof, uint8_t out[32]) {
        uint8_t m[LEAF_BYTES];
        memcpy(m, "RCKZGPROOFLEAF_1", 16);
        memcpy(m + 16, commitment, 48);
        memcpy(m + 64, z, 32);
        memcpy(m + 96, y, 32);
        memcpy(m + 128, proof, 48);
        Sha256 sh;
        sh.update(m, sizeof m);
        sh.finish(out);
    }
    // leaves: the n_p digests of the pass in the caller's order, 32 bytes each
    static void seed(uint64_t n_p, const uint8_t* leaves, uint8_t out[32]) {
        uint8_t hdr[24];
        memcpy(hdr, "RCKZGPROOFFOLD_1", 16);
        be64(n_p, hdr + 16);
        Sha256 sh;
        sh.update(hdr, sizeof hdr);
        sh.update(leaves, (size_t)n_p * 32);
        sh.finish(out);
    }
};
// the passes of a call of n items cut at `pass` items: the pass that begins at item lo ends in front of the item returned
inline uint64_t point_pass_end(uint64_t n, uint64_t lo, uint64_t pass) { return n - lo > pass ? lo + pass : n; }
// the status of an item in the single call's order of checks: the points first (commitment, then proof), then z, then y
inline int point_item_status(bool commitment_bad, bool proof_bad, const uint8_t* z, const uint8_t* y) {
    if (commitment_bad || proof_bad) return 2;
    if (geq_mod<FrParams>(fr_words_from_be(z).v) || geq_mod<FrParams>(fr_words_from_be(y).v)) return 1;
    return 0;
}

// ---- eth_kzg_amd_verify_blob_kzg_proof_many / _many_device (point_many.hip, the blob source): MANY items (blob, commitment, proof), a
// verdict for each -- exactly what Verifier::verify_blob_kzg_proof (crates/eip4844/src/verifier.rs:49-74) says of the item alone.
// There is NO new transcript: item i of a pass becomes the point item (C_i, z_i, y_i, pi_i) of PointProofTranscript above with
//     z_i = blob_challenge(blob_i, commitment_i)   hashed from the caller's bytes as they stand, also when they are invalid; the leaf
//                                                  takes its 32 canonical big-endian bytes
//     y_i = p_i(z_i)                               32 canonical big-endian bytes (k_ntt.hip: k_blob_eval_at); 32 zero bytes if the blob
//                                                  is refused
// and leaves, seed, weights, pairs, the full-range check and the search are the point path's, unchanged; a call is cut into passes of at
// most BLOB_MANY_PASS items (the host form stages 128 KB per item in the pass slot's pinned slab).
// Soundness is the point path's.  The equation checked per item is over exactly (C, z, y, pi), and the leaves bind all four, so the
// argument above holds word for word: no weight is known before every byte of (C_i, z_i, y_i, pi_i) of every item of the pass is fixed.
// That z and y are not the caller's takes nothing from it -- the prover of a wrong item still has to fix C_i and pi_i (and with them,
// through the blob, z_i and y_i) before rho_i exists -- and it is what makes the item's equation the statement about the BLOB: z and y
// are computed by the verifier from the blob's and the commitment's bytes, never supplied, exactly as in the single call.
// The one new statement is the status of an item, in the single call's order of checks (Engine::verify_blob_kzg_proof_host: the blob is
// opened first, then verify_kzg_proof_host decodes the commitment, then the proof; z is a reduced digest and y an evaluation, so neither
// can be out of range): 1 if the blob holds an element >= r -- also when a point is bad as well --, else 2 if the commitment or the proof
// is not a canonical point of the subgroup, else 0.  Only items of status 0 are live: they alone enter the sums, and only they can be
// verified.  commitment_status / proof_status: what the decoding left, 0 = a canonical point of the subgroup (k_point_many.hip:
// k_pm_blob_status is the kernel's copy).
constexpr uint64_t BLOB_MANY_MAX_ITEMS = 1u << 24;
constexpr int BLOB_MANY_PASS = 256;  // the product's pass size for the blob source (32 MB of slab); not part of the contract
inline int blob_item_status(bool blob_bad, int commitment_status, int proof_status) {
    if (blob_bad) return 1;
    if (commitment_status != 0 || proof_status != 0) return 2;
    return 0;
}
inline bool blob_item_live(int status) { return status == 0; }
// what the call hands out for an item: its status, and the pass's verdict on it only if it is live
inline bool blob_item_verified(int status, bool pair_passed) { return blob_item_live(status) && pair_passed; }

// ---- eth_kzg_amd_verify_blob_cell_proofs_many / _many_device (verify_many.hip, the blob source of the cell many-verification): MANY items
// (blob, commitment, 128 cell proofs), a verdict for each.  Item i is the problem (128 x commitment_i, indices 0..127,
// compute_cells(blob_i), proofs_i) of the many-verification under the leaf-hashed challenge of that problem alone (CellLeafTranscript,
// cell_leaf_root): there is NO new transcript, and the leaves bind the computed cells, the caller's commitment bytes and the caller's
// proofs.  Cells 0..63 are the blob's bytes, cells 64..127 come from k_ntt.hip: k_blob_to_extension (zero bytes if the blob is refused).
// Lengths and indices hold by construction: no item is refused at validation (there is no status 3), every problem has N_CELLS cells
// and ONE unique commitment with every row 0.  What the call refuses as a whole, before the context is touched:
constexpr uint64_t BLOB_CELLS_MAX_ITEMS = 1u << 24;
inline int validate_blob_cells_call(uint64_t n, bool blobs_null, bool commitments_null, bool proofs_null, bool verified_null) {
    if (n > BLOB_CELLS_MAX_ITEMS) return INPUT_INVALID;
    if (n != 0 && (blobs_null || commitments_null || proofs_null || verified_null)) return INPUT_INVALID;
    return INPUT_VALID;
}
// The status of an item, in the order of checks of the reference's two calls (compute_cells opens the blob; verify_cell_kzg_proof_batch
// then decodes the commitment and the proofs; the cells it is handed are compute_cells' own and cannot be out of range): 1 if the blob
// holds an element >= r -- also when a point is bad as well --, else 2 if the commitment or one of the 128 proofs is not a canonical
// point of the subgroup, else 0.  Only items of status 0 are live.  (The other sources of the pass decide points first: their cells are
// the caller's.)
inline int blob_cells_item_status(bool blob_bad, bool point_bad) {
    if (blob_bad) return 1;
    if (point_bad) return 2;
    return 0;
}
// Where item i of a pass lies in the pass's cells (arena and pinned slab alike, from the first cell's byte on): the layout is the
// other sources' -- cell k of item i is cell 128 i + k -- so the blob's bytes are the first half of the item's slice and the second
// half is the kernel's to fill.  Only the blob halves are staged and uploaded.
struct BlobCellsSlice { size_t blob_at, ext_at; };
inline BlobCellsSlice blob_cells_slice(size_t i) { return {i * 2 * (size_t)BYTES_PER_BLOB, (i * 2 + 1) * (size_t)BYTES_PER_BLOB}; }
static_assert(2 * BYTES_PER_BLOB == N_CELLS * BYTES_PER_CELL, "a blob is half of its 128 cells");
// the items of a call as the pass's plans see them: N_CELLS cells each (vm_call_parts, vm_chunk_end: at most chunk_cells / 128 per pass)
inline uint64_t blob_cells_of(uint64_t) { return (uint64_t)N_CELLS; }

}  // namespace kzg
