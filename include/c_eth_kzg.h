/*
 * c_eth_kzg.h -- C ABI of the MI355X-native KZG engine.
 *
 * Drop-in for the header cbindgen generates for the reference's `c_eth_kzg` crate
 * (reference: bindings/c/build.rs:24-29; symbols in bindings/c/src/lib.rs, mirrored by
 * bindings/nim/nim_code/nim_eth_kzg/header.nim and bindings/csharp/.../native_methods.g.cs).
 * Every `eth_kzg_*` prototype below has the reference's exact signature and calling
 * convention; the citation after each one is the Rust definition it replaces.
 * The `eth_kzg_amd_*` entry points are non-breaking additions: batched and
 * device-resident forms of the same operations, which is what a GPU needs to be fed.
 *
 * Ownership: inputs are borrowed for the duration of the call; outputs are written into
 * caller-allocated memory; only `CResult.error_msg` and the context are library-allocated
 * (free with eth_kzg_free_error_message / eth_kzg_das_context_free).
 * Threading: a context may be used from many threads at once.  Prover calls take one of several scratch sets; the
 * recovery / commitment / EIP-4844 calls run on up to $ETH_KZG_AMD_SERIAL_LANES (default 4) engine lanes that the context
 * creates on demand, so calls from different threads overlap on the GPU; of concurrent eth_kzg_verify_cell_kzg_proof_batch
 * callers one at a time takes the latency path and those that arrive meanwhile are combined into many-verification passes
 * behind the ABI (three pass slots; same verdicts and error split).
 */
#ifndef C_ETH_KZG_H
#define C_ETH_KZG_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bindings/c/src/lib.rs:119-123 */
typedef enum CResultStatus {
    Ok,
    Err,
} CResultStatus;

/* bindings/c/src/lib.rs:128-132 */
typedef struct CResult {
    CResultStatus status;
    char *error_msg;
} CResult;

/* bindings/c/src/lib.rs:50-52 (opaque) */
typedef struct DASContext DASContext;

/* bindings/c/src/lib.rs:79-92.  use_precomp = true selects precomputed window tables (the reference: width 8,
 * RECOMMENDED_PRECOMP_WIDTH, on the CPU; here the widest tables that fit in HBM: a GLV table of 16-bit windows for FK20,
 * 206 GB, and one of nine windows for commitments, 35 GB, when $ETH_KZG_AMD_TABLE_GB=max; by default the tables take 108 GB
 * -- nine windows each --; narrower automatically when memory is short or the budget bounds them), false the 2.4 GB sixteen-window tables and nothing wider (the
 * tables a use_precomp = true context starts on); results are identical.
 * Progressive start: the call returns as soon as small start tables are up (about 0.5 s) and every entry point works from
 * then on; the wide tables are built by a helper thread, in pieces of under a gigabyte so that no other HIP call of the process
 * waits long, and taken into use group by group (eth_kzg_amd_tables_ready, eth_kzg_amd_table_groups_ready;
 * $ETH_KZG_AMD_PROGRESSIVE=0 builds them before returning).  The embedded mainnet trusted setup is loaded; GPU 0 (or the
 * ordinal in $ETH_KZG_AMD_DEVICE) is used.  Aborts if no MI355X-class GPU is usable: there is no CPU fallback. */
DASContext *eth_kzg_das_context_new(bool use_precomp);

/* bindings/c/src/lib.rs:109-116.  NULL-safe. */
void eth_kzg_das_context_free(DASContext *ctx);

/* bindings/c/src/lib.rs:171-180.  NULL-safe. */
void eth_kzg_free_error_message(char *c_message);

/* bindings/c/src/lib.rs:196-205 -> blob_to_kzg_commitment.rs:8-38.
 * blob: 131072 bytes; out: 48 bytes. */
CResult eth_kzg_blob_to_kzg_commitment(const DASContext *ctx, const uint8_t *blob, uint8_t *out);

/* bindings/c/src/lib.rs:226-236 -> compute_cells_and_kzg_proofs.rs:8-33.
 * out_cells: 128 pointers to 2048-byte buffers; out_proofs: 128 pointers to 48-byte buffers. */
CResult eth_kzg_compute_cells_and_kzg_proofs(const DASContext *ctx, const uint8_t *blob, uint8_t **out_cells,
                                             uint8_t **out_proofs);

/* bindings/c/src/lib.rs:255-263 */
CResult eth_kzg_compute_cells(const DASContext *ctx, const uint8_t *blob, uint8_t **out_cells);

/* bindings/c/src/lib.rs:309-335 -> verify_cells_and_kzg_proofs_batch.rs:9-49.
 * commitments: one 48-byte commitment per cell (NOT deduplicated). An invalid proof is
 * `Ok` with *verified = false; malformed input is `Err` (lib.rs:272-280). A zero length means
 * the matching pointer is not dereferenced. */
CResult eth_kzg_verify_cell_kzg_proof_batch(const DASContext *ctx, uint64_t commitments_length,
                                            const uint8_t *const *commitments, uint64_t cell_indices_length,
                                            const uint64_t *cell_indices, uint64_t cells_length,
                                            const uint8_t *const *cells, uint64_t proofs_length,
                                            const uint8_t *const *proofs, bool *verified);

/* bindings/c/src/lib.rs:366-386 -> recover_cells_and_kzg_proofs.rs:10-39 */
CResult eth_kzg_recover_cells_and_proofs(const DASContext *ctx, uint64_t cells_length, const uint8_t *const *cells,
                                         uint64_t cell_indices_length, const uint64_t *cell_indices,
                                         uint8_t **out_cells, uint8_t **out_proofs);

/* bindings/c/src/lib.rs:395-405 */
uint64_t eth_kzg_constant_bytes_per_cell(void);
uint64_t eth_kzg_constant_bytes_per_proof(void);
uint64_t eth_kzg_constant_cells_per_ext_blob(void);

/* EIP-4844 single-point operations (bindings/c/src/lib.rs:423-566 -> compute_kzg_proof.rs, compute_blob_kzg_proof.rs,
 * verify_kzg_proof.rs, verify_blob_kzg_proof.rs, verify_blob_kzg_proof_batch.rs), on the same GPU kernels.
 * z, y: 32-byte big-endian field elements; invalid proof => `Ok` + *verified = false; malformed input => `Err`. */
CResult eth_kzg_compute_kzg_proof(const DASContext *ctx, const uint8_t *blob, const uint8_t *z, uint8_t *out_proof,
                                  uint8_t *out_y);
CResult eth_kzg_compute_blob_kzg_proof(const DASContext *ctx, const uint8_t *blob, const uint8_t *commitment,
                                       uint8_t *out_proof);
CResult eth_kzg_verify_kzg_proof(const DASContext *ctx, const uint8_t *commitment, const uint8_t *z, const uint8_t *y,
                                 const uint8_t *proof, bool *verified);
CResult eth_kzg_verify_blob_kzg_proof(const DASContext *ctx, const uint8_t *blob, const uint8_t *commitment,
                                      const uint8_t *proof, bool *verified);
CResult eth_kzg_verify_blob_kzg_proof_batch(const DASContext *ctx, uint64_t blobs_length, const uint8_t *const *blobs,
                                            uint64_t commitments_length, const uint8_t *const *commitments,
                                            uint64_t proofs_length, const uint8_t *const *proofs, bool *verified);

/* ---------------------------------------------------------------------------------------------
 * MI355X additions (no counterpart in the reference; its single-blob ABI cannot feed a GPU).
 * Status arrays receive one int per blob: 0 ok, 1 = a field element >= r, 2 = bad G1 point,
 * 3 = invalid input, 4 = recovery failed.  The CResult is `Err` only for call-level failures.
 */

/* Context on an explicit GPU ordinal (one process per GPU under torch.distributed/RCCL). */
DASContext *eth_kzg_amd_das_context_new_on_device(bool use_precomp, int device_ordinal);

/* The constructor that never kills the host process.  eth_kzg_das_context_new keeps the reference's behaviour -- the Rust
 * constructor panics across the FFI when it cannot build a context (bindings/c/src/lib.rs:79-92), this library aborts when there
 * is no usable GPU or not even the 2.4 GB start tables fit -- which is hostile inside a consensus client.  This form returns NULL
 * and fills *result (status Err, error_msg to be freed with eth_kzg_free_error_message; may be NULL) instead; on success *result
 * is Ok.  table_budget_gb bounds the HBM the two window tables take together: > 0 = that many GB (the commitment table takes the
 * widest GLV table within a third of it, the FK20 table the widest within the rest: 108 GB -> nine windows each, 44 -> ten, 22 ->
 * eleven, 3 -> sixteen), 0 = $ETH_KZG_AMD_TABLE_GB or else the default of 108 GB (-7 % against the widest tables at 44 % of their
 * memory), < 0 = whatever the HBM still holds (242 GB on an idle GPU: eight windows of 16 bits for FK20, nine for commitments). */
DASContext *eth_kzg_amd_das_context_try_new(bool use_precomp, int device_ordinal, double table_budget_gb, CResult *result);

/* A context over a DEVICE LIST: one engine per listed GPU behind the one pointer, so that a host written against the
 * reference -- one context, shared by all its threads (bindings/c/src/lib.rs:79-92, bindings/node/src/lib.rs:35,75,
 * bindings/golang/prover.go) -- uses every GPU of the node through the UNCHANGED sixteen symbols:
 *   - a single-problem call (eth_kzg_compute_cells_and_kzg_proofs, _verify_cell_kzg_proof_batch, _recover_cells_and_proofs,
 *     _blob_to_kzg_commitment, the EIP-4844 calls) runs on the device with the least work in flight;
 *   - a host-pointer batch (eth_kzg_amd_*_batch, _verify_cell_kzg_proof_batch_many) is cut into contiguous slices, slice d =
 *     [n d / D, n (d + 1) / D) on the d-th listed device, one host thread each, the caller's buffers are the gather target
 *     (no collective); the call's error is the lowest failing device's;
 *   - a device-resident call (eth_kzg_amd_*_device) runs on the listed device that owns the caller's buffers (`Err` if none does);
 *   - the communicator, profiling and table-introspection calls address the FIRST listed device (eth_kzg_amd_table_bytes sums
 *     the distinct devices, eth_kzg_amd_tables_ready reports the slowest one).
 * Results are byte-identical to a one-device context's.  eth_kzg_das_context_new reads the list from ETH_KZG_AMD_DEVICES
 * ("0,1,2,3" or "all"; unset: ETH_KZG_AMD_DEVICE, else GPU 0).  An ordinal may repeat (two engines on one GPU share its window
 * tables): the form the one-GPU tests use.  Returns NULL and fills *result (as _try_new) when any device fails. */
DASContext *eth_kzg_amd_das_context_new_on_devices(bool use_precomp, const int32_t *device_ordinals, uint64_t n_devices,
                                                   double table_budget_gb, CResult *result);
/* the context's device list: writes up to `capacity` ordinals, returns how many devices the context spans */
uint64_t eth_kzg_amd_context_devices(const DASContext *ctx, int32_t *out_ordinals, uint64_t capacity);
/* Version of the eth_kzg_amd_* additions (the sixteen eth_kzg_* symbols never change): 6 = this header.  Bumped whenever a
 * symbol's meaning changes or one is removed, so that an out-of-tree consumer can check at load time. */
int eth_kzg_amd_abi_version(void);

/* ---- a caller-supplied trusted setup ----
 * Every other constructor builds the context on the mainnet ceremony file that is linked into the library.  Chains with a
 * ceremony of their own, devnets and test suites (an insecure setup with a known secret) hand their points in here -- the
 * reference's DASContext::new(&TrustedSetup, ..) with TrustedSetup::from_json / from_json_unchecked
 * (crates/eip7594/src/lib.rs:81, crates/trusted_setup/src/lib.rs:88-124), c-kzg's load_trusted_setup.
 *   g1_monomial   n_g1 = 4096 points [tau^i]_1, 48 bytes each, ZCash compressed (the JSON's "g1_monomial"; NOT "g1_lagrange")
 *   g2_monomial   n_g2 = 65 points [tau^i]_2, 96 bytes each
 *   flags         ETH_KZG_AMD_SETUP_*; 0 = what from_json does
 *   device_ordinals / n_devices   a device list as for eth_kzg_amd_das_context_new_on_devices; NULL and 0: the devices
 *                 eth_kzg_das_context_new would pick (ETH_KZG_AMD_DEVICES / ETH_KZG_AMD_DEVICE / GPU 0)
 *   table_budget_gb   as eth_kzg_amd_das_context_try_new
 * Never aborts: NULL and Err("ContextCreation(..)") otherwise.  The counts, the pointers and the flags are checked before a GPU is
 * looked for ("InvalidInput: a trusted setup holds 4096 G1 and 65 G2 monomial points, got .."); other sizes are not supported.
 * Validation of the points ("InvalidSetup: g1_monomial[2077] is not in the prime-order subgroup" -- the FIRST bad index is named):
 *   - every point must be the canonical compressed encoding of a curve point; a point at infinity in g1_monomial is refused;
 *   - every G1 point (on the GPU, endomorphism test) and every G2 point (on the host, psi-endomorphism test) must lie in the
 *     subgroup of order r, unless ETH_KZG_AMD_SETUP_NO_SUBGROUP_CHECK (from_json_unchecked) is given.  Unchecked, g1_monomial[1]
 *     must still be in the subgroup: the library calibrates its endomorphism on it;
 *   - ETH_KZG_AMD_SETUP_CHECK_POWERS: g1_monomial[0] and g2_monomial[0] are the standard generators and both lists are
 *     consecutive powers of one tau (two random-weight pairing checks; error 2^-128).  This is what catches a well-formed file
 *     in the wrong basis or order -- Lagrange points passed as monomial ones pass every subgroup test and give wrong proofs.
 *     Off by default (the reference has no such check); costs two 4096-point MSMs on the GPU and four pairings;
 *   - a setup from which a base at infinity is derived is refused ("degenerate trusted setup"): an FK20 base, or the verification
 *     base [tau^64 - h^64]_2 of a coset -- tau inside the evaluation domain (tau^8192 = 1; tau = 1 is the plain case), where
 *     every proof for that coset's cell would verify.
 * Everything else is as for the embedded setup: progressive start, table budget, use_precomp, device lists, serial lanes.  The
 * window tables are shared between the contexts of a GPU that hold the SAME setup (equal eth_kzg_amd_setup_digest) and only
 * those; the mainnet points handed in here give the same bytes as eth_kzg_das_context_new in every output and share its tables. */
#define ETH_KZG_AMD_SETUP_NO_SUBGROUP_CHECK 1u
#define ETH_KZG_AMD_SETUP_CHECK_POWERS 2u
DASContext *eth_kzg_amd_das_context_new_with_setup(const uint8_t *g1_monomial, uint64_t n_g1, const uint8_t *g2_monomial,
                                                   uint64_t n_g2, uint32_t flags, bool use_precomp,
                                                   const int32_t *device_ordinals, uint64_t n_devices,
                                                   double table_budget_gb, CResult *result);
/* The same from ONE buffer in the flat layout of rust-eth-kzg_amd/data/trusted_setup_4096.bin:
 * "KZGSRS01" | n_g1 (u32, little endian) | n_g2 (u32) | n_g1 * 48 bytes | n_g2 * 96 bytes.  Forwards to the constructor above. */
DASContext *eth_kzg_amd_das_context_new_with_setup_file(const uint8_t *file, uint64_t file_length, uint32_t flags,
                                                        bool use_precomp, const int32_t *device_ordinals,
                                                        uint64_t n_devices, double table_budget_gb, CResult *result);
/* Which setup a context holds: SHA-256 over the g1_monomial bytes followed by the g2_monomial bytes (32 bytes out). */
void eth_kzg_amd_setup_digest(const DASContext *ctx, uint8_t *out_digest /* 32 */);

/* Host-pointer batches: n blobs; out_cells[b] / out_proofs[b] are arrays of 128 pointers as in the
 * single-blob calls (either may be NULL to skip that output). */
CResult eth_kzg_amd_compute_cells_and_kzg_proofs_batch(const DASContext *ctx, uint64_t n, const uint8_t *const *blobs,
                                                       uint8_t *const *const *out_cells,
                                                       uint8_t *const *const *out_proofs, int32_t *status);
CResult eth_kzg_amd_blob_to_kzg_commitment_batch(const DASContext *ctx, uint64_t n, const uint8_t *const *blobs,
                                                 uint8_t *const *out, int32_t *status);

/* n independent recoveries in one pass (BASELINE.json config 5). Blob b supplies cells_lengths[b] cells
 * (cells[b][k], 2048 B each) with indices cell_indices[b][k]; outputs as in the batch call above. status[b] = 0 ok,
 * 1 a cell holds a non-canonical field element, 3 invalid indices / counts, 4 the cells are not consistent. */
CResult eth_kzg_amd_recover_cells_and_proofs_batch(const DASContext *ctx, uint64_t n, const uint64_t *cells_lengths,
                                                   const uint8_t *const *const *cells,
                                                   const uint64_t *cell_indices_lengths,
                                                   const uint64_t *const *cell_indices, uint8_t *const *const *out_cells,
                                                   uint8_t *const *const *out_proofs, int32_t *status);

/* Device-resident recovery (BASELINE.json config 5 for pipelines that hold extended blobs in HBM): d_cells is the flat
 * [n][128][2048] layout on this GPU; present_masks (HOST memory) holds two 64-bit words per blob, bit (c % 64) of word
 * (c / 64) set when cell c carries data - missing cells are never read.  Replaces the cell list + index list of
 * eth_kzg_recover_cells_and_proofs (bindings/c/src/lib.rs:366): ascending unique indices hold by construction, a blob
 * needs at least 64 present cells.  Outputs as in eth_kzg_amd_compute_cells_and_kzg_proofs_device (either may be NULL);
 * status[b] (HOST, n entries) = 0 ok, 1 non-canonical field element, 3 fewer than 64 cells, 4 cells not consistent with
 * a degree < 4096 polynomial; outputs of a failed blob are unspecified.  The decode runs on the library's stream, ordered
 * after the work already queued on hip_stream (event) and completed before the call returns (the status words come back
 * from it); the cells and proofs kernels are enqueued on hip_stream behind it (NULL: library stream, synchronised). */
CResult eth_kzg_amd_recover_cells_and_proofs_device(const DASContext *ctx, uint64_t n, const uint8_t *d_cells,
                                                    const uint64_t *present_masks, uint8_t *d_out_cells,
                                                    uint8_t *d_out_proofs, int32_t *status, void *hip_stream);

/* verify_cell_kzg_proof_batch sharded over GPUs (BASELINE.json config 3).  The verification
 * equation of crates/cryptography/kzg_multi_open/src/fk20/verifier.rs:139-260 is linear in the cells once the
 * Fiat-Shamir challenge (taken over the WHOLE batch) is fixed, so each rank evaluates its slice
 * [shard_begin, shard_end) of the cell list and emits a 96-byte record (two compressed G1 partial sums);
 * the records of all ranks are all-gathered and handed to _combine, which adds them and runs the one pairing check.
 * Arguments before shard_begin are exactly those of eth_kzg_verify_cell_kzg_proof_batch and must describe the whole
 * batch on every rank.  Malformed input in the rank's slice (or in the shared lengths / indices) => Err.
 * The union of the slices must be [0, cells_length); an empty slice is fine. */
#define ETH_KZG_AMD_VERIFY_PARTIAL_BYTES 96
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_partial(const DASContext *ctx, uint64_t commitments_length,
                                                        const uint8_t *const *commitments, uint64_t cell_indices_length,
                                                        const uint64_t *cell_indices, uint64_t cells_length,
                                                        const uint8_t *const *cells, uint64_t proofs_length,
                                                        const uint8_t *const *proofs, uint64_t shard_begin,
                                                        uint64_t shard_end, uint8_t *out_partial /* 96 */);
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_combine(const DASContext *ctx, uint64_t n_partials,
                                                        const uint8_t *partials /* n_partials * 96 */, bool *verified);

/* MANY independent verifications in one call -- the throughput form of eth_kzg_verify_cell_kzg_proof_batch (the reference gets
 * its throughput by verifying from many threads on one context, bindings/node/src/lib.rs:92-299).  Problem b is described by
 * commitments[b] / cell_indices[b] / cells[b] / proofs[b] with the four lengths *_lengths[b], exactly as one call of the
 * single form; the problems share every GPU launch (one lane per scalar multiplication), their transcripts are hashed on host
 * threads in parallel, and the pairing checks of a pass are folded into one with 127-bit weights derived from all the
 * challenges (error 2^-127, the argument of the powers of r inside one batch); in a pass that contains wrong proofs they are
 * found by folding sub-ranges of the resident weighted sums (a handful of pairings per wrong proof instead of one per problem)
 * down to single problems, so a false verdict is always exact and per problem.  Where a level of that search holds many probes their
 * pairings run on the GPU, one per lane (ETH_KZG_AMD_GPU_PAIRING_MIN; neither verdicts nor statuses depend on it).  A problem may hold at most 2^24 - 1 cells.  Per problem: status[b] = 0 and verified[b] = the verdict, or
 * status[b] = 1 (a cell holds a non-canonical field element), 2 (bad G1 encoding / not in the subgroup), 3 (invalid lengths
 * or indices) and verified[b] = false -- what the single form reports as Err (status may be NULL).  The CResult is Err only
 * for a call-level (device) failure.  An empty problem verifies (verifier.rs:90-93). */
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_many(const DASContext *ctx, uint64_t n_batches,
                                                     const uint64_t *commitments_lengths,
                                                     const uint8_t *const *const *commitments,
                                                     const uint64_t *cell_indices_lengths,
                                                     const uint64_t *const *cell_indices, const uint64_t *cells_lengths,
                                                     const uint8_t *const *const *cells, const uint64_t *proofs_lengths,
                                                     const uint8_t *const *const *proofs, bool *verified, int32_t *status);

/* Device-resident batches: flat buffers already in this GPU's HBM.
 *   d_blobs        n * 131072 bytes
 *   d_out_cells    n * 128 * 2048 bytes   (may be NULL)
 *   d_out_proofs   n * 128 * 48 bytes     (may be NULL)
 *   d_out          n * 48 bytes
 *   status         n ints in HOST memory, or NULL: then nothing is copied back and, if
 *                  `hip_stream` is non-NULL, the call returns without synchronising (work is
 *                  enqueued on that hipStream_t; NULL = the context's own stream, synchronised).
 * Inputs produced by work the caller has queued on `hip_stream` are waited for on the device; with NULL that is the
 * work queued so far on the DEFAULT stream (the library's own streams are non-blocking streams: without this a kernel
 * of the caller's default stream that writes d_blobs could still be running when the call reads them).
 * Calls on one stream are ordered.  The context owns a few sets of intermediate buffers; a call takes a free one and
 * makes its stream wait for the previous user of that set, so asynchronous calls on different streams are safe too
 * (they overlap while sets are free, otherwise they queue). */
CResult eth_kzg_amd_compute_cells_and_kzg_proofs_device(const DASContext *ctx, uint64_t n, const uint8_t *d_blobs,
                                                        uint8_t *d_out_cells, uint8_t *d_out_proofs, int32_t *status,
                                                        void *hip_stream);
CResult eth_kzg_amd_blob_to_kzg_commitment_device(const DASContext *ctx, uint64_t n, const uint8_t *d_blobs,
                                                  uint8_t *d_out, int32_t *status, void *hip_stream);

/* The EIP-4844 proofs for MANY blobs in one call -- the throughput forms of eth_kzg_compute_kzg_proof and
 * eth_kzg_compute_blob_kzg_proof (bindings/c/src/lib.rs:423-480 -> crates/eip4844/src/prover.rs:37-92), which prove one blob per call
 * with an upload, a launch set and a synchronisation each.  Per blob they compute what the single calls compute, byte for byte.
 * status[b] follows the single call's order of checks: 1 = the blob holds a field element >= r, else 1 = z is not canonical
 * (compute_kzg_proof) or 2 = the commitment is not a valid point of the subgroup (compute_blob_kzg_proof; it is only validated,
 * prover.rs:73-75), else 0.  The outputs of a blob whose status is not 0 are unspecified (host forms: left untouched).
 *
 * Host-pointer forms: n pointers each -- blobs[b] 131072 bytes, commitments[b] / out_proofs[b] 48, zs[b] / out_ys[b] 32 (big-endian,
 * as in the single call).  The blobs are gathered into pinned memory and the Fiat-Shamir challenges
 * z_b = H("FSBLOBVERIFY_V1_" | 4096 | blob_b | commitment_b) (crates/eip4844/src/verifier.rs:155-196) hashed by host threads in
 * parallel (the bytes are on the host already), then every 256 blobs are one upload and one set of launches.  status may be NULL. */
CResult eth_kzg_amd_compute_blob_kzg_proof_batch(const DASContext *ctx, uint64_t n, const uint8_t *const *blobs,
                                                 const uint8_t *const *commitments, uint8_t *const *out_proofs,
                                                 int32_t *status);
CResult eth_kzg_amd_compute_kzg_proof_batch(const DASContext *ctx, uint64_t n, const uint8_t *const *blobs,
                                            const uint8_t *const *zs, uint8_t *const *out_proofs, uint8_t *const *out_ys,
                                            int32_t *status);
/* Device-resident forms: flat arrays in this GPU's HBM -- d_blobs n * 131072 bytes, d_commitments / d_out_proofs n * 48, d_zs /
 * d_out_ys n * 32 big-endian (4-byte aligned) -- for pipelines that already hold their blobs there (commitments from
 * eth_kzg_amd_blob_to_kzg_commitment_device): nothing but the status words crosses the link.  The challenges of the blob proofs
 * are hashed ON THE GPU, one lane per blob (csrc/k_sha256.hip): the 131 KB of a blob do not come down for a 32-byte answer.  That
 * hash is serial inside a blob and takes a few milliseconds whatever n is: for a handful of blobs the
 * host-pointer form or the single call is the faster one.  status, hip_stream, ordering behind the caller's queued work and
 * asynchronous use exactly as eth_kzg_amd_blob_to_kzg_commitment_device above (status NULL and a stream given: the call returns
 * without synchronising). */
CResult eth_kzg_amd_compute_blob_kzg_proof_device(const DASContext *ctx, uint64_t n, const uint8_t *d_blobs,
                                                  const uint8_t *d_commitments, uint8_t *d_out_proofs, int32_t *status,
                                                  void *hip_stream);
CResult eth_kzg_amd_compute_kzg_proof_device(const DASContext *ctx, uint64_t n, const uint8_t *d_blobs, const uint8_t *d_zs,
                                             uint8_t *d_out_proofs, uint8_t *d_out_ys, int32_t *status, void *hip_stream);
/* eth_kzg_verify_blob_kzg_proof_batch (bindings/c/src/lib.rs:530-566 -> crates/eip4844/src/verifier.rs:80-196) on flat arrays in this
 * GPU's HBM: n * 131072 blob bytes, n * 48 commitment bytes, n * 48 proof bytes.  Challenges (GPU hash) and evaluations y_b are
 * computed where the blobs lie, commitments and proofs are decompressed in place; the n * (48 + 32 + 32 + 48) bytes of the
 * "RCKZGBATCH___V1_" transcript come down and the weight r is hashed on the host (one short serial message), then the two bucket
 * MSMs and the pairing check as in the host form.  Synchronous; work already queued on `hip_stream` (NULL: the default stream)
 * that produces the inputs is waited for.  Verdict and errors as the host form: Err for a non-canonical blob element, else a bad
 * commitment, else a bad proof; n = 0 verifies.  ONE random linear combination over the whole batch: never cut over a device list. */
CResult eth_kzg_amd_verify_blob_kzg_proof_batch_device(const DASContext *ctx, uint64_t n, const uint8_t *d_blobs,
                                                       const uint8_t *d_commitments, const uint8_t *d_proofs, bool *verified,
                                                       void *hip_stream);

/* MANY eth_kzg_verify_kzg_proof items in one call, A VERDICT FOR EACH: the throughput form of the check behind the point-evaluation
 * precompile, for callers that hold (commitment, z, y, proof) tuples and need to know WHICH of them is wrong (the batch call above
 * computes z and y from blobs and gives one verdict for all).  Item i: commitments[i] / proofs[i] -> 48 bytes, zs[i] / ys[i] -> 32
 * bytes big-endian.  Per item the result is exactly what eth_kzg_verify_kzg_proof says of that item alone, in its order of checks
 * (crates/eip4844/src/verifier.rs:19-44):
 *   status[i] = 2  the commitment or the proof is not a canonical point of the subgroup (also when z or y is bad as well),
 *   else      = 1  z or y is >= r,
 *   else      = 0  and verified[i] is the verdict.  verified[i] is false whenever status[i] != 0.  status may be NULL.
 * The call: n = 0 is Ok; n > 2^24, or a NULL array with n > 0, is Err("InvalidInput...") before the context is touched; otherwise Err
 * only for a device failure.  How: csrc/verify_host.hpp (PointProofTranscript) states the check once -- the items of a pass (at most
 * 16384; not part of the contract) are hashed into leaves, the leaves into a seed, the seed into a 127-bit weight rho_i per item, and
 * ONE pairing check of  ( sum rho_i pi_i , sum rho_i (C_i + z_i pi_i - y_i G) )  over the pass's valid items passes only if every
 * one of them is valid (error 2^-127: no weight is known before every input byte is fixed); if it fails the wrong items are searched
 * by checking the pairs of sub-ranges down to single items, and a single item whose own pair fails is wrong exactly.  Where a level of
 * that search holds many probes their pairings run on the GPU, one per lane (ETH_KZG_AMD_GPU_PAIRING_MIN; neither
 * verdicts nor statuses depend on it).  The scalar
 * multiplications run one lane each on the GPU (csrc/k_point_many.hip), the pass on a pass slot of the many-verification: the call
 * does not take the context's big lock and runs next to every other entry point.  The identity is a valid commitment and a valid proof.
 * Host form: cut into contiguous slices by item over the context's device list; the host threads hash the leaves.
 * Device form: flat arrays in this GPU's HBM -- the 48-byte arrays from any byte address, d_zs / d_ys 4-byte aligned (as
 * eth_kzg_amd_compute_kzg_proof_device) -- verified / status HOST memory.  Synchronous; work already queued on `hip_stream` (NULL: the
 * default stream) is waited for.  The GPU hashes the leaves: nothing but the status words, the n x 32 leaf digests and the sums come
 * down, and only the weights go up.  Runs on the device that owns the buffers: all four pointers are resolved, and anything but device
 * memory of ONE device of the context is Err("InvalidInput...").  When it pays: INTEGRATION.md. */
CResult eth_kzg_amd_verify_kzg_proof_many(const DASContext *ctx, uint64_t n, const uint8_t *const *commitments,
                                          const uint8_t *const *zs, const uint8_t *const *ys, const uint8_t *const *proofs,
                                          bool *verified, int32_t *status);
CResult eth_kzg_amd_verify_kzg_proof_many_device(const DASContext *ctx, uint64_t n, const uint8_t *d_commitments, const uint8_t *d_zs,
                                                 const uint8_t *d_ys, const uint8_t *d_proofs, bool *verified, int32_t *status,
                                                 void *hip_stream);

/* MANY eth_kzg_verify_blob_kzg_proof items in one call, A VERDICT FOR EACH: the throughput form of the blob check for callers that need
 * to know WHICH blob of a batch is wrong (eth_kzg_verify_blob_kzg_proof_batch / _batch_device give one verdict for all, and a node whose
 * batch fails would otherwise fall back to one single call per blob).  Item i: blobs[i] -> 131072 bytes, commitments[i] / proofs[i] -> 48
 * bytes.  Per item the result is exactly what eth_kzg_verify_blob_kzg_proof says of that item alone, in its order of checks
 * (crates/eip4844/src/verifier.rs:49-74):
 *   status[i] = 1  the blob holds a field element >= r (also when a point is bad as well),
 *   else      = 2  the commitment or the proof is not a canonical point of the subgroup,
 *   else      = 0  and verified[i] is the verdict.  verified[i] is false whenever status[i] != 0.  status may be NULL.
 * The identity is a valid commitment and a valid proof: the all-zero blob with two identities verifies.
 * The call: n = 0 is Ok; n > 2^24, or a NULL array with n > 0, is Err("InvalidInput...") before the context is touched; otherwise Err
 * only for a device failure, and then every verified[i] is false.
 * How: there is no new transcript.  Item i becomes the point item (C_i, z_i, y_i, pi_i) of eth_kzg_amd_verify_kzg_proof_many above, with
 * z_i = H("FSBLOBVERIFY_V1_" | 4096 | blob_i | commitment_i) mod r hashed from the caller's bytes as they stand and y_i = p_i(z_i)
 * evaluated on the GPU without leaving the CU (csrc/k_ntt.hip: k_blob_eval_at -- one block per blob: the inverse transform in LDS, then
 * the 4096 coefficients are summed against powers of z where they lie; no coefficient and no quotient is written to HBM); y_i is 32 zero
 * bytes for a refused blob.  Leaves, seed, weights, the one pairing check per pass and the search are that call's, unchanged (the
 * search's pairings on the GPU from ETH_KZG_AMD_GPU_PAIRING_MIN probes per level included), and so is
 * the soundness argument (csrc/verify_host.hpp): the per-item equation is over exactly (C, z, y, pi), all of which the leaves bind, and
 * z and y are computed by the verifier, not supplied.  The leaves are hashed on the GPU in both forms (y exists only there).  A pass
 * holds at most 256 items (not part of the contract) and runs on a pass slot: the call does not take the context's big lock, needs
 * none of the prover's workspace and runs next to every other entry point; a call of several passes uses up to three slots.
 * Host form: cut into contiguous slices by item over the context's device list; the helper threads gather a pass's blobs into pinned
 * memory and hash the challenges while the bytes are in their cache; one upload per pass.
 * Device form: flat arrays in one GPU's HBM -- d_blobs n * 131072, d_commitments / d_proofs n * 48 bytes, with the alignment
 * eth_kzg_amd_verify_blob_kzg_proof_batch_device asks for (the 48-byte arrays from any byte address) -- verified / status HOST memory.
 * The blobs are read where they lie and never copied; the challenges are hashed on the GPU, one lane per blob, which takes a few
 * milliseconds whatever n is.  Synchronous; work already queued on `hip_stream` (NULL: the default stream) is waited for.  Runs on the
 * device that owns the buffers: all three pointers are resolved, and anything but device memory of ONE device of the context is
 * Err("InvalidInput...").  The Node binding is not extended.  When it pays: INTEGRATION.md. */
CResult eth_kzg_amd_verify_blob_kzg_proof_many(const DASContext *ctx, uint64_t n, const uint8_t *const *blobs,
                                               const uint8_t *const *commitments, const uint8_t *const *proofs, bool *verified,
                                               int32_t *status);
CResult eth_kzg_amd_verify_blob_kzg_proof_many_device(const DASContext *ctx, uint64_t n, const uint8_t *d_blobs,
                                                      const uint8_t *d_commitments, const uint8_t *d_proofs, bool *verified,
                                                      int32_t *status, void *hip_stream);

/* MANY blobs against their 128 CELL PROOFS in one call, A VERDICT FOR EACH: the throughput form of the check a blob transaction gets since
 * PeerDAS (EIP-7594), where the wire carries the blob, its commitment and the blob's 128 cell proofs and the transaction pool checks
 * cells = compute_cells(blob), then verify_cell_kzg_proof_batch([commitment] * 128, [0..127], cells, proofs).  Item i: blobs[i] -> 131072
 * bytes, commitments[i] -> 48 bytes, proofs[i][k] -> 48 bytes for k < 128.  Item i gets the verdict that
 * eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex with ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT gives the problem (128 x commitments[i], indices
 * 0..127, compute_cells(blobs[i]), proofs[i]); the statuses follow the order of checks of the reference's two calls, compute_cells first:
 *   status[i] = 1  the blob holds a field element >= r (also when a point of the item is bad as well),
 *   else      = 2  the commitment or one of the 128 proofs is not a canonical point of the subgroup,
 *   else      = 0  and verified[i] is the verdict.  verified[i] is false whenever status[i] != 0.  status may be NULL.
 * There is no status 3: lengths and indices hold by construction.  The identity is a valid commitment and a valid proof: the all-zero
 * blob with 129 identities verifies.
 * The call: n = 0 is Ok; n > 2^24, or a NULL array with n > 0, is Err("InvalidInput...") before the context is touched; otherwise Err
 * only for a device failure, and then every verified[i] is false.
 * How: there is no flags word and no new transcript.  The blobs are a fourth SOURCE of the many-verification's pass
 * (csrc/verify_many.hip): blob i's bytes are cells 0..63 of its problem as they stand, and cells 64..127 are computed behind them in the
 * pass's arena without leaving the CU (csrc/k_ntt.hip: k_blob_to_extension -- one block per blob: the inverse transform, the twist and the
 * forward transform on one image in LDS; no coefficient is written to HBM and none of the prover's workspace is used); a refused blob
 * gets zero bytes there.  The challenge of item i is always the leaf-hashed one of that problem alone, exactly as _many_ex takes it under
 * the flag, the leaves hashed on the GPU out of the arena: they bind the computed cells, the caller's commitment bytes and the caller's
 * proofs.  The folding weights, the one pairing check per pass and the search (its pairings on the GPU from
 * ETH_KZG_AMD_GPU_PAIRING_MIN probes per level) keep their form.  A verdict never depends on the challenge, and the caller never sees
 * it; the soundness paragraph of eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex carries over unchanged.
 * The call runs on pass slots (at most 1024 blobs per pass, three parts side by side from 192 blobs on; not part of the contract): it
 * does not take the context's big lock, needs none of the prover's work sets and runs next to every other entry point.
 * Host form: cut into contiguous slices by item over the context's device list; per pass the blobs and proofs are gathered into pinned
 * memory and uploaded -- 128 KB + 6 KB per blob up, nothing but status words, leaf digests and sums down -- where
 * compute_cells_and_kzg_proofs_batch + _many_ex move 256 KB of cells down and up again and 56 x 128 bytes of commitments and indices.
 * Device form: flat arrays in one GPU's HBM -- d_blobs n * 131072 bytes with the alignment
 * eth_kzg_amd_verify_blob_kzg_proof_many_device asks for, d_commitments n * 48 and d_proofs n * 128 * 48 bytes from any byte address --
 * verified / status HOST memory.  One device-to-device copy per pass brings the blobs into the arena; only the n * 48 commitment bytes
 * come down.  Synchronous; work already queued on `hip_stream` (NULL: the default stream) is waited for.  Runs on the device that owns
 * the buffers: all three pointers are resolved, and anything but device memory of ONE device of the context is Err("InvalidInput...").
 * Out of scope: interpolation sums taken straight from the coefficients in place of the per-cell interpolation; writing the decoded
 * evaluations from the new kernel and skipping the cells' decoding; a reference-transcript variant; _partial / _combine; sharding a device
 * form over GPUs.  The Node binding is not extended.  When it pays: INTEGRATION.md. */
CResult eth_kzg_amd_verify_blob_cell_proofs_many(const DASContext *ctx, uint64_t n, const uint8_t *const *blobs,
                                                 const uint8_t *const *commitments, const uint8_t *const *const *proofs, bool *verified,
                                                 int32_t *status);
CResult eth_kzg_amd_verify_blob_cell_proofs_many_device(const DASContext *ctx, uint64_t n, const uint8_t *d_blobs,
                                                        const uint8_t *d_commitments, const uint8_t *d_proofs, bool *verified,
                                                        int32_t *status, void *hip_stream);

/* verify_cell_kzg_proof_batch on flat arrays in this GPU's HBM: n * 48 commitment bytes (one per cell, NOT deduplicated, as in
 * the host form), n indices, n * 2048 cell bytes, n * 48 proof bytes.  The GPU's part reads cells and proofs where they are;
 * the transcript hash runs on a host core, so its bytes come down (in chunks, under the hash) and the call is synchronous;
 * work already queued on `hip_stream` (NULL: the default stream) that produces the inputs is waited for.  Result and error behaviour as eth_kzg_verify_cell_kzg_proof_batch. */
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_device(const DASContext *ctx, uint64_t n, const uint8_t *d_commitments,
                                                       const uint64_t *d_cell_indices, const uint8_t *d_cells,
                                                       const uint8_t *d_proofs, bool *verified, void *hip_stream);

/* ---- cell verification with a leaf-hashed challenge ----
 * The reference's Fiat-Shamir transcript is ONE SHA-256 over every byte of the batch: serial by construction, and for a large batch
 * the time of the whole call is the time of that hash on one host core (8192 cells: 17.6 MB).  Only the verdict crosses this ABI --
 * the challenge r never does -- so the two calls below take, when asked to, a challenge that binds the same bytes through a
 * two-level hash whose first level runs on the GPU, one lane per cell (csrc/k_sha256.hip):
 *   LEAF_k = SHA-256("RCKZGCBATCHLEAF1" | be64(k) | be64(cell_indices[k]) | commitments[k] | proofs[k] | cells[k])
 *   ROOT   = SHA-256("RCKZGCBATCHROOT1" | be64(4096) | be64(64) | be64(n) | LEAF_0 | .. | LEAF_{n-1})
 *   r      = ROOT as a 256-bit big-endian integer mod r
 * (k: the position in the caller's list; commitments[k]: the caller's 48 bytes of entry k, not de-duplicated.)
 * Soundness: r is a hash of every input byte -- the leaves bind the contents, the root binds their order, and the argument rests on
 * the collision resistance of SHA-256.  The batch equation is the reference's: a batch that holds a wrong proof passes only if r is
 * a root of a non-zero polynomial of degree below n over Fr.  Valid batches verify under any r, and whether a call is Err or
 * Ok(false) does not depend on r: validation, the order in which errors are reported (commitments, proofs, cells) and the
 * pairing check are those of the unflagged calls.
 *   flags = 0                                    exactly eth_kzg_verify_cell_kzg_proof_batch / eth_kzg_amd_verify_cell_kzg_proof_batch_device
 *   flags = ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT   the challenge above.  In the device-resident form neither cells nor proofs are
 *                                                copied to the host: the commitments and the indices come down (validation and
 *                                                de-duplication), and the n * 32 digest bytes
 *   any other bit                                Err("InvalidInput..."), returned with the count checks, before the context is touched
 * On a device-list context the host form routes like any single-problem call, the device form by the owner of the pointers.
 * Not covered: eth_kzg_amd_verify_cell_kzg_proof_batch_partial / _combine and the combining of concurrent calls of
 * eth_kzg_verify_cell_kzg_proof_batch keep the reference's transcript; no environment setting moves the reference's own symbol
 * onto this challenge.  The many-verification takes the flag through its own _ex calls, below.  When the flag pays: INTEGRATION.md. */
#define ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT 1u
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_ex(const DASContext *ctx, uint64_t commitments_length,
                                                   const uint8_t *const *commitments, uint64_t cell_indices_length,
                                                   const uint64_t *cell_indices, uint64_t cells_length,
                                                   const uint8_t *const *cells, uint64_t proofs_length,
                                                   const uint8_t *const *proofs, uint32_t flags, bool *verified);
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_device_ex(const DASContext *ctx, uint64_t n, const uint8_t *d_commitments,
                                                          const uint64_t *d_cell_indices, const uint8_t *d_cells,
                                                          const uint8_t *d_proofs, uint32_t flags, bool *verified,
                                                          void *hip_stream);

/* ---- the many-verification with a flags word, and on flat arrays in HBM ----
 * eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex: eth_kzg_amd_verify_cell_kzg_proof_batch_many with a flags word: 0 = exactly that
 * call; ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT = every problem's challenge is the leaf-hashed one.
 * eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex: the same on flat arrays in this GPU's HBM.  cell_starts: HOST,
 * n_batches + 1 entries, cell_starts[0] = 0, non-decreasing; problem b is the entries [cell_starts[b], cell_starts[b+1]) of the four
 * arrays; N = cell_starts[n_batches].  d_commitments N*48 (one per cell, NOT de-duplicated, as in the single device form),
 * d_cell_indices N uint64, d_cells N*2048, d_proofs N*48.  Any byte address for the byte arrays.  verified / status: HOST, n_batches
 * entries (status may be NULL).  Synchronous; work already queued on hip_stream (NULL: the default stream) that produces the inputs is
 * waited for.
 * The challenge of a problem under the flag is exactly what eth_kzg_amd_verify_cell_kzg_proof_batch_ex would take for that problem
 * alone: k in LEAF_k is the position INSIDE the problem (it restarts at 0 in each one), ROOT carries the problem's own n,
 * commitments[k] are the caller's 48 bytes; there are no new domain strings.  All the leaves of a pass are hashed in one launch, one
 * lane per cell; the host hashes one ROOT per problem.  The folding weights that let one pairing check stand for a whole pass keep
 * their form (SHA-256 under "RCKZGCBATCHFOLD1" over the problems' digests, then per problem); under the flag the digests are the
 * problems' ROOTs in the place of the reference transcript's digests, and a problem that is empty or refused at validation contributes
 * 32 zero bytes, as before.  The soundness paragraph above carries over: every ROOT is a hash of every input byte of its problem, so
 * the weights still hang on every input byte of the pass and are fixed only after all of them.
 * Verdicts and statuses: per problem status 0 / 1 / 2 / 3 in the reference's error order (commitments, proofs, cells) and verified,
 * exactly as _many; whether a problem is refused, false or true does not depend on the flag; an empty problem verifies.  In the device
 * form the four lengths of a problem are one by construction, so status 3 is left for an index >= 128 or more than 2^24 - 1 cells.
 * Err("InvalidInput...") for the call, checked before the context is touched: a bit other than the leaf flag; n_batches > 2^24; a
 * malformed cell_starts (NULL with n_batches > 0, a first entry that is not 0, a decreasing entry).  n_batches = 0 is Ok.
 *   device form, flags = 0      the reference's challenges: the pass copies its proofs and cells down into pinned memory and hashes them
 *                               on the host threads as the host form does.  Correct, and the slow way: it is there so that the flag
 *                               means the same in every _ex call and so that the resident pass can be compared with the host pass
 *                               byte for byte, not for speed.
 *   device form, leaf flag      neither cells nor proofs cross the link: the commitments and indices come down for validation and
 *                               de-duplication (56 bytes per cell), then the n * 32 leaf digests, the status words and the sums.
 * Device lists: the host form is cut by problem over the listed devices, exactly as _many; the device form runs on the device that owns
 * the buffers, and all four device pointers are resolved: Err("InvalidInput...") unless they are device memory of one listed device.
 * Out of scope: _partial / _combine keep the reference's transcript; so does the combiner of concurrent
 * eth_kzg_verify_cell_kzg_proof_batch callers; the Node binding is not extended; no environment setting moves the unflagged calls;
 * the caller's cells are not read in place -- the pass copies them device-to-device into its arena, as the single resident form does
 * (2 KB per cell at HBM speed, against milliseconds of pass).  Measured figures: INTEGRATION.md. */
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex(const DASContext *ctx, uint64_t n_batches,
                                                        const uint64_t *commitments_lengths, const uint8_t *const *const *commitments,
                                                        const uint64_t *cell_indices_lengths, const uint64_t *const *cell_indices,
                                                        const uint64_t *cells_lengths, const uint8_t *const *const *cells,
                                                        const uint64_t *proofs_lengths, const uint8_t *const *const *proofs,
                                                        uint32_t flags, bool *verified, int32_t *status);
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex(const DASContext *ctx, uint64_t n_batches, const uint64_t *cell_starts,
                                                               const uint8_t *d_commitments, const uint64_t *d_cell_indices,
                                                               const uint8_t *d_cells, const uint8_t *d_proofs, uint32_t flags,
                                                               bool *verified, int32_t *status, void *hip_stream);

/* ---- the data columns of one block, the commitments given once ----
 * A PeerDAS data column sidecar is one cell index, and for every blob of the block one cell and one proof; the block's n_blobs
 * commitments are the same for every column.  eth_kzg_amd_verify_data_columns takes them ONCE:
 *   commitments[i]    48 B, blob i                      column_indices[j]   the cell index of column j
 *   cells[j][i]       2048 B, the cell of blob i in column j              proofs[j][i]   48 B
 * eth_kzg_amd_verify_data_columns_device: the same in this GPU's HBM -- d_commitments n_blobs*48, d_cells [n_columns][n_blobs][2048],
 * d_proofs [n_columns][n_blobs][48], any byte address; column_indices, verified and status on the HOST.  Synchronous; work already
 * queued on hip_stream (NULL: the default stream) is waited for.
 * Contract: column j gets exactly the verified[j] and status[j] that eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex gives a problem
 * with the n_blobs commitments as given (one per cell), n_blobs copies of column_indices[j], cells[j] and proofs[j] -- in the
 * reference's order of checks: status 3 for an index >= 128 or n_blobs > 2^24 - 1; else 2 for a bad commitment, which therefore marks
 * EVERY column 2; else 2 for a bad proof of that column; else 1 for a non-canonical cell of that column; else 0 and the verdict.
 * verified[j] is false whenever status[j] != 0; status may be NULL.  n_columns = 0 is Ok.  n_blobs = 0 makes every column verify
 * whatever its index (an empty problem is validated without an index being read).  Indices may repeat and come in any order;
 * commitments may repeat.
 *   flags = 0                                    the reference's transcript per column
 *   flags = ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT   the leaf-hashed challenge, exactly as the flagged single call takes it for that column
 *                                                alone; no new domain strings, no new transcript, the folding weights keep their form
 * Err("InvalidInput...") for the call, before the context is touched: any other flag bit; n_columns > 2^24; a NULL array with a non-zero
 * count (commitments, cells or proofs with n_blobs > 0 and n_columns > 0 -- also when n_blobs is beyond the bound; column_indices or
 * verified with n_columns > 0).  A column refused at validation costs its status word: it is taken out of the call before any pass.  Device form: all three device pointers are resolved -- anything but device memory of one listed device is Err; the
 * commitments come down once (48 * n_blobs bytes); under the leaf flag neither cells nor proofs cross the link, with flags = 0 they
 * come down for the host's hashes as in _many_device_ex.  Device lists: the host form is cut by column over the listed devices, the
 * device form runs on the owner of the buffers.
 * What the call saves against _many on the expanded input is work, not meaning: the unique commitments are decoded and subgroup-tested
 * once per pass (not once per column), and the cells of a column share h^64, so the second proof product is one per column
 * (h^64 * sum_k r^k proof_k) where the expanded pass runs one per cell.  Fewer operations, NOT a faster call at the sizes measured:
 * that one product is a dependent launch and 128 columns x 64 blobs take 0.8 ms longer than _many_device_ex on the expanded input
 * (DESIGN.md section 5).  The call is there for its interface; when to take it: INTEGRATION.md.
 * Out of scope: one inverse transform per column in the place of the per-cell interpolation; cheaper w*C products over the shared
 * points; reading the caller's cells in place; _partial / _combine; the combiner of concurrent single calls; the Node binding. */
CResult eth_kzg_amd_verify_data_columns(const DASContext *ctx, uint64_t n_blobs, const uint8_t *const *commitments,
                                        uint64_t n_columns, const uint64_t *column_indices,
                                        const uint8_t *const *const *cells, const uint8_t *const *const *proofs,
                                        uint32_t flags, bool *verified, int32_t *status);
CResult eth_kzg_amd_verify_data_columns_device(const DASContext *ctx, uint64_t n_blobs, const uint8_t *d_commitments,
                                               uint64_t n_columns, const uint64_t *column_indices, const uint8_t *d_cells,
                                               const uint8_t *d_proofs, uint32_t flags, bool *verified, int32_t *status,
                                               void *hip_stream);

/* ---- partial data columns: a bitmap of the blobs present per column ----
 * Cell-level dissemination does not send whole sidecars: a partial data column sidecar carries a column index, a bitmap of the blobs
 * present, and cells and proofs for those blobs only.  eth_kzg_amd_verify_partial_data_columns checks many such messages of one block
 * over the block's commitment list, given ONCE:
 *   commitments[i]   48 B, blob i (all n_blobs of the block)      column_indices[j]   the cell index of column j
 *   present[j]       W = ceil(n_blobs / 64) words; bit i % 64 of word i / 64 is set when column j carries blob i (the convention of
 *                    present_masks in eth_kzg_amd_recover_cells_and_proofs_device).  m_j = the set bits among the first n_blobs
 *   cells[j][k] / proofs[j][k], k < m_j: of the k-th set bit in ascending blob order
 * eth_kzg_amd_verify_partial_data_columns_device: d_commitments n_blobs*48, d_cells [N][2048] and d_proofs [N][48] PACKED in this GPU's
 * HBM, any byte address: column after column, within a column ascending blob order.  A column occupies as many entries as ALL W of its
 * words have set bits, stray bits included (so a refused column is skipped without being read); N is the sum of these counts.
 * column_indices, present (flat, [n_columns][W]), verified and status are on the HOST.  Synchronous; work already queued on hip_stream
 * (NULL: the default stream) is waited for.
 * Contract: column j gets exactly the verified[j] and status[j] that eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex gives the problem
 * (commitments[i] for the set bits i in ascending order; m_j copies of column_indices[j]; cells[j]; proofs[j]), under either flag value:
 * no new transcript, no new domain string, the folding weights keep their form.  Order of checks per column: status 3 for n_blobs >
 * 2^24 - 1 (every column, nothing read), a set bit at or beyond n_blobs, or m_j > 0 and an index >= 128; else 2 when a commitment OF A
 * PRESENT BLOB is bad -- a bad commitment marks the columns that hold a cell of that blob and no others, one that no column holds marks
 * nothing --; else 2 for a bad proof of the column; else 1 for a non-canonical cell of the column; else 0 and the verdict.
 * verified[j] is false whenever status[j] != 0; status may be NULL.  A column with no bit set verifies whatever its index (an empty
 * problem).  Indices may repeat: two messages for one column with disjoint bitmaps are two problems.  Commitments may repeat.
 * n_columns = 0 is Ok.  flags: 0 = the reference's transcript per column, ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT as in the dense call.
 * Err("InvalidInput...") for the call, before the context is touched: any other flag bit; n_columns > 2^24; column_indices or verified
 * NULL with n_columns > 0; present NULL with n_columns > 0 and n_blobs > 0; commitments, cells or proofs NULL with both counts non-zero.
 * A column refused at validation costs its status word: it is taken out of the call before any pass.  Device lists: the host form is cut
 * by column over the listed devices; the device form runs on the owner of the buffers, and all three device pointers are resolved.
 * The call de-duplicates the block's commitments once, a pass decodes each unique commitment once, every proof is multiplied once
 * (the column shares h^64), and weights and w*C products exist only for the (column, commitment) pairs that hold a cell.
 * Reconstruction from partial columns needs nothing new: per-blob erasure patterns are what
 * eth_kzg_amd_recover_cells_and_proofs_batch takes.
 * Out of scope: recovery in a masked column layout; merging partial columns; _partial / _combine; the combiner of concurrent single
 * calls; sharding a device form over GPUs; the Node binding. */
CResult eth_kzg_amd_verify_partial_data_columns(const DASContext *ctx, uint64_t n_blobs, const uint8_t *const *commitments,
                                                uint64_t n_columns, const uint64_t *column_indices, const uint64_t *const *present,
                                                const uint8_t *const *const *cells, const uint8_t *const *const *proofs,
                                                uint32_t flags, bool *verified, int32_t *status);
CResult eth_kzg_amd_verify_partial_data_columns_device(const DASContext *ctx, uint64_t n_blobs, const uint8_t *d_commitments,
                                                       uint64_t n_columns, const uint64_t *column_indices, const uint64_t *present,
                                                       const uint8_t *d_cells, const uint8_t *d_proofs,
                                                       uint32_t flags, bool *verified, int32_t *status, void *hip_stream);

/* ---- a block's data columns computed and recovered in column layout ----
 * The two neighbours of eth_kzg_amd_verify_data_columns, in its layout: cells and proofs as [column][blob], which is how the 128 data
 * column sidecars of a block carry them, so that a caller transposes nothing between the three calls.
 *   out_cells[c][i] / d_out_cells [128][n_blobs][2048]    cell c of blob i        out_proofs[c][i] / d_out_proofs [128][n_blobs][48]
 *
 * eth_kzg_amd_compute_data_columns / _device -- the proposer's call: everything the sidecars of a block carry, from its blobs.
 * Contract: for blob i, status[i], the commitment and the bytes of cell c and proof c are exactly what
 * eth_kzg_amd_blob_to_kzg_commitment_batch and eth_kzg_amd_compute_cells_and_kzg_proofs_batch (device form: the _device forms of the
 * two) give for blob i at cell c.  Each of the three outputs may be NULL and is then not computed; status may be NULL.  A blob with
 * status 1 (an element >= r) leaves its own slots untouched in the host form and unspecified in the device form, and disturbs no other
 * blob's bytes.  Device form: status on the HOST; stream, ordering behind the caller's queued work, asynchronous return and alignment
 * as eth_kzg_amd_compute_cells_and_kzg_proofs_device -- with status == NULL and a stream given the call returns without synchronising.
 * How: the blobs are decoded ONCE per sub-batch -- one launch leaves the coefficients in the form the proofs' stages read and in the
 * canonical form the commitment's fixed-base MSM reads, where the two separate calls decode every blob twice -- and the kernels that
 * write cells and proofs store every byte once, at its column address: there is no transposition pass and no [blob][128] copy.
 *
 * eth_kzg_amd_recover_data_columns / _device -- the supernode's call: all 128 columns from n_columns >= 64 of them.
 *   column_indices[j]  HOST, the cell index of the j-th column given, strictly ascending
 *   cells[j][i] / d_cells [n_columns][n_blobs][2048]      the cell of blob i in that column
 * Contract: for blob i, status[i] and the bytes are exactly what eth_kzg_amd_recover_cells_and_proofs_batch gives for the list
 * (cells[0][i] .. cells[n_columns-1][i], column_indices).  A bad index list -- fewer than 64 or more than 128 entries, not strictly
 * ascending, an index >= 128 -- therefore marks EVERY blob 3, before anything is launched.  A non-canonical element gives status 1 for
 * its blob only, an inconsistent cell status 4 for its blob only; outputs of such a blob: untouched (host form), unspecified (device
 * form).  out_cells / out_proofs may be NULL.  Device form: streams and synchronisation as eth_kzg_amd_recover_cells_and_proofs_device:
 * the decode runs on the library's stream behind what hip_stream has queued and has completed when the call returns.
 * How: every blob of a block misses the same columns, so ONE vanishing polynomial is built and evaluated per call, not one per blob;
 * the present cells are read where they lie in the column matrix, and the outputs are written at their column addresses.
 *
 * Err("InvalidInput...") for the call, before the context is touched: n_blobs > 2^24; a NULL array with a non-zero count (blobs; cells;
 * column_indices with n_columns > 0; status in the recover forms).  n_blobs = 0 is Ok.
 * Device lists: the host forms are cut into contiguous slices by BLOB over the listed devices, the caller's pointers being the gather
 * target as in the other batched calls; the device forms run on the device that owns the buffers -- all device pointers given are
 * resolved, and anything but device memory of one listed device is Err("InvalidInput...").
 * Out of scope: passing present columns through instead of recomputing them; returning only the missing columns; sharding a device
 * form over GPUs; the Node binding.  When to take the calls, and what was measured: INTEGRATION.md, DESIGN.md section 5. */
CResult eth_kzg_amd_compute_data_columns(const DASContext *ctx, uint64_t n_blobs, const uint8_t *const *blobs,
                                         uint8_t *const *out_commitments, uint8_t *const *const *out_cells,
                                         uint8_t *const *const *out_proofs, int32_t *status);
CResult eth_kzg_amd_compute_data_columns_device(const DASContext *ctx, uint64_t n_blobs, const uint8_t *d_blobs,
                                                uint8_t *d_out_commitments, uint8_t *d_out_cells, uint8_t *d_out_proofs,
                                                int32_t *status, void *hip_stream);
CResult eth_kzg_amd_recover_data_columns(const DASContext *ctx, uint64_t n_blobs, uint64_t n_columns,
                                         const uint64_t *column_indices, const uint8_t *const *const *cells,
                                         uint8_t *const *const *out_cells, uint8_t *const *const *out_proofs, int32_t *status);
CResult eth_kzg_amd_recover_data_columns_device(const DASContext *ctx, uint64_t n_blobs, uint64_t n_columns,
                                                const uint64_t *column_indices, const uint8_t *d_cells, uint8_t *d_out_cells,
                                                uint8_t *d_out_proofs, int32_t *status, void *hip_stream);

/* ---- a block's data columns from blobs whose cell proofs the caller HOLDS ----
 * eth_kzg_amd_blobs_to_data_columns / _device -- the call of a proposer, and of every node that fetches blobs from its execution client
 * (getBlobsV2), the transaction pool or a relay: since PeerDAS a blob arrives with its 128 cell proofs, so the node that builds the 128
 * sidecars runs no FK20.  It needs cells = compute_cells(blob) as [column][blob], the proofs it was handed re-ordered from [blob][128]
 * to [128][blob], and usually a check of those proofs before it signs or forwards anything.
 *   blobs[i] / d_blobs n_blobs * 131072      commitments[i] / d_commitments n_blobs * 48      proofs[i][k] / d_proofs [n_blobs][128][48]
 *   out_cells[c][i] / d_out_cells [128][n_blobs][2048]      out_proofs[c][i] / d_out_proofs [128][n_blobs][48]
 * out_cells / out_proofs may each be NULL and are then not produced.  verified and status are HOST memory.
 * flags = 0: status[i] is what eth_kzg_amd_compute_data_columns gives blob i (1: an element >= r, else 0) and out_cells[c][i] are the
 * bytes of that call's out_cells[c][i]; out_proofs[c][i] are the 48 bytes of proofs[i][c] as they stand -- never decoded: garbage is
 * copied as garbage.  commitments is not read and may be NULL; verified is not written and may be NULL; status may be NULL.  Device
 * form: status, stream, ordering behind the caller's queued work and alignment of d_blobs as eth_kzg_amd_compute_data_columns_device
 * (d_out_cells 4-byte aligned like d_blobs; d_proofs and d_out_proofs from any byte address); with status == NULL and a stream given
 * the call returns without synchronising.
 * flags = ETH_KZG_AMD_COLUMNS_VERIFY_PROOFS: status[i] and verified[i] are exactly what eth_kzg_amd_verify_blob_cell_proofs_many /
 * _many_device give item i -- that call's order of checks, its leaf-hashed challenge per item, its folding weights, its one pairing
 * check per pass, its search and its soundness paragraph; there is no new transcript and no new domain string.  Synchronous; runs on
 * pass slots and does not take the context's big lock.
 * Outputs.  Host form: blob i's slots are written only when status[i] == 0 and, under the flag, verified[i] is true; otherwise they
 * stay as the caller left them.  Device form: the slots of such a blob are unspecified.  No other blob's bytes are disturbed.
 * Err("InvalidInput...") for the call, before the context is touched: any other flag bit; n_blobs > 2^24; blobs NULL with n_blobs > 0;
 * proofs NULL when the flag is set or out_proofs is given; commitments or verified NULL when the flag is set.  n_blobs = 0 is Ok.
 * Device lists: the host form is cut into contiguous slices by blob; the device form runs on the owner of the buffers -- every device
 * pointer given is resolved, and anything but device memory of one listed device is Err("InvalidInput...").
 * How.  flags = 0: one block per blob computes all 128 cells without leaving the CU (csrc/k_ntt.hip: k_blob_to_columns, the image and
 * transforms of k_blob_to_extension) and stores every byte once at its column address -- no coefficient goes to HBM, none of the
 * prover's workspace is used and there is no [blob][128] intermediate -- and one small kernel re-orders the proofs.  Host form: every
 * blob is uploaded once and only cells 64..127 (128 KB per blob) come down; cells 0..63 ARE the caller's blob bytes and out_proofs the
 * caller's proof bytes, copied on the host by the helper threads.  Under the flag the columns are an output of the blob source of the
 * many-verification (csrc/verify_many.hip): the pass keeps its blob-major arena for leaves and decoding, a copy kernel behind the
 * extension step puts the cells at their column addresses (device form) or the extension halves come down into the pass's pinned slab
 * (host form), and the proofs are re-ordered from where the pass holds them.  Each blob is uploaded once where the two calls it
 * replaces upload it twice and extend it twice.
 * Out of scope: computing missing proofs with FK20 inside this call; computing or checking commitments from the blobs; a
 * reference-transcript variant; sharding a device form over GPUs.  The Node binding is not extended.  When it pays: INTEGRATION.md. */
#define ETH_KZG_AMD_COLUMNS_VERIFY_PROOFS 1u
CResult eth_kzg_amd_blobs_to_data_columns(const DASContext *ctx, uint64_t n_blobs, const uint8_t *const *blobs,
                                          const uint8_t *const *commitments, const uint8_t *const *const *proofs, uint32_t flags,
                                          uint8_t *const *const *out_cells, uint8_t *const *const *out_proofs, bool *verified,
                                          int32_t *status);
CResult eth_kzg_amd_blobs_to_data_columns_device(const DASContext *ctx, uint64_t n_blobs, const uint8_t *d_blobs,
                                                 const uint8_t *d_commitments, const uint8_t *d_proofs, uint32_t flags,
                                                 uint8_t *d_out_cells, uint8_t *d_out_proofs, bool *verified, int32_t *status,
                                                 void *hip_stream);

/* ---- a block's data columns recovered AND checked against the block's commitments ----
 * eth_kzg_amd_recover_data_columns / _device cannot tell a right input from a wrong one when exactly 64 columns are given: the decoder's
 * only consistency test is that the recovered polynomial has no coefficient at 4096 or above (status 4), and ANY 64 columns of
 * canonical bytes decode to some polynomial of degree below 4096 -- status 0, with 128 cells and 128 proofs that are valid for a
 * polynomial nobody committed to.  What identifies the right polynomial is the block's commitment, and the recovered coefficients are in
 * HBM when the decode ends: the checked forms commit to them (one fixed-base MSM per blob, the stages of
 * eth_kzg_amd_blob_to_kzg_commitment_device) and compare.
 *   commitments[i] / d_commitments n_blobs*48          the commitment blob i is expected to have; NULL: nothing is compared
 *   out_blobs[i] / d_out_blobs [n_blobs][131072]       the recovered blob, blob-major: its cells 0..63 concatenated
 *   out_commitments[i] / d_out_commitments n_blobs*48  the commitment of the recovered polynomial
 *   column_indices, cells, out_cells, out_proofs, status, hip_stream: as eth_kzg_amd_recover_data_columns / _device
 * Status of blob i, in this order: 3 a bad index list -- it marks EVERY blob, before anything is launched and before commitments is
 * read (device form: before any pointer is resolved); else 1 a non-canonical element in the blob's cells; else 4 the cells lie on no
 * polynomial of degree below 4096; else 6 the recovered polynomial's commitment differs from commitments[i]; else 0.  The statuses 0, 1,
 * 3 and 4 are exactly what eth_kzg_amd_recover_data_columns gives on the same cells, whatever the commitments are.  6 is a value no
 * other call returns (5 is taken inside the library).
 * The comparison is on BYTES: the computed commitment in its canonical 48-byte compressed encoding against the caller's 48 bytes as
 * they stand.  The caller's commitment is never decoded, so a malformed or non-canonical one -- flag bits wrong, x not below p, a point
 * off the curve or outside the subgroup -- can never match: it gives 6, NOT 2.  The identity (0xc0 00 ... 00) matches the all-zero blob
 * and nothing else.  With commitments == NULL status 6 cannot occur.
 * Outputs.  Blob with status 0: out_cells / out_proofs hold the bytes of eth_kzg_amd_recover_data_columns, out_commitments[i] the bytes
 * eth_kzg_amd_blob_to_kzg_commitment_batch gives for the recovered blob, out_blobs[i] that blob's own 131072 bytes.  Any other status:
 * the blob's slots are untouched (host form) or unspecified (device form); no other blob's bytes are disturbed.  Each of the four
 * outputs may be NULL and is then not computed.  With all four NULL the call is a pure check: the decode, the commitments and the
 * comparison, no cell kernel and no FK20 stage.  With commitments and out_commitments NULL as well it is the decode and the statuses of
 * eth_kzg_amd_recover_data_columns and nothing more.
 * What status 0 says when commitments are given.  The decoder's test passed: the quotient Q it recovered has degree below 4096, so Q Z
 * (Z the vanishing polynomial of the missing cells, degree at most 4096) has degree below 8192 and agrees with the interpolant of E Z on
 * the 8192 points of the coset; hence Q Z = E Z on the domain itself, and every GIVEN cell is Q's evaluation.  commit(Q) == C_i then
 * identifies Q as the committed polynomial under the binding of KZG.  So status 0 says of every given cell what a valid cell proof
 * says of it -- at least 64 columns of a block checked against the commitments WITHOUT any proofs.  What the call cannot do is name the
 * wrong column: a blob with 4 or 6 goes through eth_kzg_amd_verify_data_columns, with proofs, for that.
 * Err("InvalidInput...") for the call, before the context is touched: exactly what eth_kzg_amd_recover_data_columns refuses -- n_blobs >
 * 2^24, or NULL cells, column_indices (with n_columns > 0) or status with n_blobs > 0.  n_blobs = 0 is Ok.
 * Device form: every device pointer given is resolved, d_commitments, d_out_blobs and d_out_commitments included; anything but device
 * memory of one listed device is Err("InvalidInput...").  The byte arrays may start at any byte address; the caller's commitments are
 * read where they lie.  Streams as eth_kzg_amd_recover_data_columns_device: the decode, the commitments and the comparison run on the
 * library's stream behind what hip_stream has queued -- the work that wrote d_commitments included -- and have completed when the call
 * returns, d_out_commitments with them; the kernels that write d_out_blobs, d_out_cells and d_out_proofs go onto hip_stream.
 * Device lists: the host form is cut into contiguous slices by BLOB (commitments, out_blobs and out_commitments indexed like every other
 * array of the call); the device form runs on the owner of the buffers.
 * How: the last pass of the decoder stores the coefficients a second time as canonical integers; the MSM, its fold, the compression
 * and the comparison are enqueued in front of the decode's one synchronisation, so a sub-batch costs one synchronisation as before and
 * the status words come down once.  A blob whose decode failed runs through the commitment stages all the same and its result is
 * ignored.  out_blobs is the cells' transform launched for cells 0..63 alone, written blob-major.
 * Out of scope: the blob-major recovery calls (their erasure patterns differ per blob); locating the wrong column; decoding or
 * subgroup-testing the caller's commitments; passing present columns through; returning only the missing columns; sharding a device
 * form over GPUs; the Node binding.  When to take the call, and what was measured: INTEGRATION.md, DESIGN.md section 5. */
CResult eth_kzg_amd_recover_data_columns_checked(const DASContext *ctx, uint64_t n_blobs, const uint8_t *const *commitments,
                                                 uint64_t n_columns, const uint64_t *column_indices,
                                                 const uint8_t *const *const *cells, uint8_t *const *out_blobs,
                                                 uint8_t *const *out_commitments, uint8_t *const *const *out_cells,
                                                 uint8_t *const *const *out_proofs, int32_t *status);
CResult eth_kzg_amd_recover_data_columns_checked_device(const DASContext *ctx, uint64_t n_blobs, const uint8_t *d_commitments,
                                                        uint64_t n_columns, const uint64_t *column_indices, const uint8_t *d_cells,
                                                        uint8_t *d_out_blobs, uint8_t *d_out_commitments, uint8_t *d_out_cells,
                                                        uint8_t *d_out_proofs, int32_t *status, void *hip_stream);

/* Introspection used by bench.py / DESIGN.md: bytes of both window tables resident in HBM; nominal window width w of the FK20
 * table in use (a GLV table: ceil(128 / w) windows over the two 128-bit halves of each scalar, packed 96-byte entries: 16
 * gathered additions per base at w = 16, 32 at w = 8 -- the start tables, and all there is with use_precomp = false). */
uint64_t eth_kzg_amd_table_bytes(const DASContext *ctx);
/* NOMINAL: since ABI version 5 the windows of a table have mixed widths (w = 15: two windows of 15 bits and seven of 14) -- do
 * not derive the additions per base from it; eth_kzg_amd_window_count gives the windows per 128-bit GLV half directly (gathered
 * additions per base = 2 x that: 16 on the widest tables, 18 on the default ones, 32 on the start tables). */
int eth_kzg_amd_window_bits(const DASContext *ctx);
int eth_kzg_amd_window_count(const DASContext *ctx);
/* DEPRECATED (kept for consumers linked against the round-4 header): always 1 -- every window table is a GLV table now. */
int eth_kzg_amd_glv_table(const DASContext *ctx);
/* 1 once the final window tables are in use, 0 while the context still runs on its start tables (waits up to wait_ms
 * milliseconds for the switch; negative: until it happened), 2 if the wide tables could not be built (memory) and the
 * context stays on what it has.  Results never depend on the table in use. */
int eth_kzg_amd_tables_ready(const DASContext *ctx, int wait_ms);
/* The wide FK20 table is allocated in pieces of under a gigabyte and used GROUP BY GROUP while the helper thread builds it (the
 * 128 MSM groups of a blob: the groups already built run on the wide table, the rest on the start table): this returns how
 * many of the 128 groups of the table under construction are in use (128 once it is complete or when nothing is being built). */
int eth_kzg_amd_table_groups_ready(const DASContext *ctx);
/* How the window tables in use were allocated: out4[0] = milliseconds spent in hipMalloc for their pieces, out4[1] = the longest
 * single allocation (ms), out4[2] = number of pieces, out4[3] = bytes.  On an idle GPU a piece takes 2 ms; a piece that takes
 * seconds is the driver waiting for memory that another process has just freed to be wiped, and the calling process's GPU
 * queues stand still for as long (tools/alloc_test/probe_stall.cpp): the one start-up stall the library cannot remove. */
void eth_kzg_amd_table_build_info(const DASContext *ctx, double *out4);
/* The compiled linear map that replaces the two G1 transforms of the prover: out4 = constant multiplications, point
 * additions, point doublings per blob, kernel launches per call. */
void eth_kzg_amd_linmap_info(const DASContext *ctx, int32_t *out4);

/* Per-stage HIP-event timing for bench.py's roofline leg.  Stages, in order: blob_to_coeffs,
 * coeffs_to_cells, fk20_scalars, msm_fixed, g1_ifft, g1_fft, compress, g1_linmap.  get_stage_times writes the
 * milliseconds and kernel-launch counts accumulated since the previous call (it synchronises the
 * device) and returns the number of stages. */
void eth_kzg_amd_set_profiling(const DASContext *ctx, int on);
int eth_kzg_amd_get_stage_times(const DASContext *ctx, double *ms, uint64_t *launches, int n);

/* ---- multi-GPU (north_star: blob batches shard across the GPUs of a node; one all-gather of the proof vectors) ----
 *
 * (1) One process per GPU (torchrun / MPI style).  The library owns the RCCL communicator: rank 0 obtains an id,
 *     the caller distributes its 128 bytes by whatever it already has (MPI_Bcast, torch.distributed, a file), every
 *     rank attaches its context, and eth_kzg_amd_all_gather is one ncclAllGather over xGMI on the given stream:
 *     d_recv receives world * bytes_per_rank bytes, rank r's slab at offset r * bytes_per_rank.  RCCL is bound with
 *     dlopen when the first of these functions is called, so the library itself does not depend on it: a copy the
 *     process has already mapped (PyTorch ships one) is reused, otherwise librccl.so.1 is loaded.
 *     eth_kzg_amd_comm_init is COLLECTIVE (ncclCommInitRank): every rank must enter it or none; call
 *     eth_kzg_amd_comm_probe first (local, cheap: Ok iff RCCL can be bound and the context has no communicator yet;
 *     optionally reports which library file was bound) and agree on the result before any rank calls _init.
 *     eth_kzg_amd_comm_info returns the rank and size the communicator itself reports (ncclCommUserRank/Count). */
CResult eth_kzg_amd_comm_probe(const DASContext *ctx, char *out_library_path /* may be NULL */, uint64_t path_capacity);
CResult eth_kzg_amd_comm_unique_id(uint8_t *out_id /* 128 */);
CResult eth_kzg_amd_comm_init(DASContext *ctx, const uint8_t *id /* 128 */, int rank, int world);
CResult eth_kzg_amd_comm_info(const DASContext *ctx, int *out_rank, int *out_world);
CResult eth_kzg_amd_all_gather(const DASContext *ctx, const void *d_send, void *d_recv, uint64_t bytes_per_rank,
                               void *hip_stream);
void eth_kzg_amd_comm_destroy(DASContext *ctx);
/* (2) One process, several GPUs: contexts[d] created with eth_kzg_amd_das_context_new_on_device(.., d).  The batch
 *     is cut into contiguous slices, one per context, each served by its own host thread through the host-pointer
 *     path above; the caller's buffers are the gather target, so there is no collective.  status as in the batch call. */
CResult eth_kzg_amd_compute_cells_and_kzg_proofs_batch_multi(const DASContext *const *contexts, uint64_t n_contexts,
                                                             uint64_t n, const uint8_t *const *blobs,
                                                             uint8_t *const *const *out_cells,
                                                             uint8_t *const *const *out_proofs, int32_t *status);
/* number of GPUs visible to the library (hipGetDeviceCount) */
int eth_kzg_amd_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* C_ETH_KZG_H */
