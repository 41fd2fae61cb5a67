/* Stage-level hooks of libc_eth_kzg for the kernel parity tests under tests/ -- NOT part of the drop-in ABI
 * (bindings/c of the reference has nothing like them).  Kept out of c_eth_kzg.h so that consumers never see them. */
#ifndef C_ETH_KZG_TEST_HOOKS_H
#define C_ETH_KZG_TEST_HOOKS_H
#include "c_eth_kzg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* canonical big-endian encodings; return 0 on success */
int eth_kzg_amd_test_fr_ntt4096(const DASContext *ctx, const uint8_t *in, uint8_t *out, int inverse_dit);
int eth_kzg_amd_test_g1_fft128(const DASContext *ctx, const uint8_t *in, uint8_t *out, int n_lanes, int inverse);
int eth_kzg_amd_test_fixed_msm(const DASContext *ctx, const uint8_t *scalars, int n_msm, uint8_t *out);
int eth_kzg_amd_test_g1_decompress(const DASContext *ctx, const uint8_t *in, int n, int subgroup_check, int32_t *status,
                                   uint8_t *out);
int eth_kzg_amd_test_field_mul(const DASContext *ctx, const uint8_t *a, const uint8_t *b, uint8_t *out, int n,
                               int is_fp);

/* The decoded coordinates themselves (eth_kzg_amd_test_g1_decompress re-compresses on the device with the decoder's own sign predicate,
 * so a predicate that is wrong both ways still returns the input bytes).  in: n0 + n1 compressed points (host), two segments as the
 * verifiers pass proofs and commitments (n0 >= 1, n1 >= 0; forms 0 and 1 take one segment: n1 = 0).  The status words start at the
 * verifiers' 0xff poison.  Exactly the product's launch calls, nothing new on the device; with N = n0 + n1 and M = the limit of the
 * four-lanes-per-point kernels (launch::coop_points_max: 8192, ETH_KZG_AMD_COOP_POINTS moves it) the kernels of a form are:
 *   0  launch::g1_decompress, check 0: k_g1_decompress (one lane per point, no subgroup test) at every N
 *   1  launch::g1_decompress, check 1: k_g1_decompress_coop for N <= M, k_g1_decompress above
 *   2  launch::g1_decompress2:         k_g1_decompress_coop for N <= M, k_g1_decompress above
 *   3  launch::g1_decode2, then launch::g1_subgroup2: k_g1_subgroup_coop for N <= M, k_g1_subgroup above
 *   4  launch::g1_decode2, then launch::pip_shift_prepare_and_subgroup over all N points with the workspace of
 *      eth_kzg_amd_test_verify_msm: its quad branch for 2 N <= M (it counts the shifted points and the tested ones), its one-lane branch above
 * status[n0 + n1]: 0 good, 1 bad encoding or off the curve, 2 outside the subgroup (form 0: never 2).
 * out_xy[n0 + n1][96]: the affine x | y the point array holds behind the launches, canonical big-endian; 96 zero bytes for the identity.
 * The decoders (forms 0 .. 2, and the decode of 3 and 4) write the identity over a point they refuse; the subgroup-only kernels of forms 3
 * and 4 write the status word alone, so a point they refuse with 2 keeps its decoded coordinates.  A slot no kernel wrote reads 0xff.
 * Synchronous; returns 0, or the library's status codes (counts or form out of range: 3). */
int eth_kzg_amd_test_g1_decode(const DASContext *ctx, int form, const uint8_t *in, int n0, int n1, int32_t *status, uint8_t *out_xy);

/* One stated schedule of the fixed-base MSM (csrc/k_msm_glv.inc) on either window table.  table_kind: 0 = the FK20 table (128 groups of 64
 * bases), 1 = the commitment table (64 groups; the output is then the 64 group sums of a slice, before the commitment's fold).  mode: -1 =
 * what the engine picks for n_slices (launch_msm_range; its two-launch overflow form included), 0 = a block per MSM (flat), 1 = a lane per
 * window, 3 = two lanes per window, 2 = four chunks per MSM.  scalar_form: 0 = canonical big-endian scalars (32 B), split on the device as
 * eth_kzg_amd_test_fixed_msm splits them; 1 = the two balanced GLV halves themselves, 8 little-endian 32-bit words per scalar: |k1| in words
 * 0 .. 3, |k2| in words 4 .. 7, each below 2^127 with its sign in bit 127 -- word for word what the prover's Fr kernels leave
 * (eth_kzg_amd_test_prover_scalars), read through the overload the prover calls.  scalars[n_slices][groups][64] (host, 1 <= n_slices <= 4096),
 * out[n_slices][groups][48] (host).  modes[5]: modes[0] = launches made, modes[1 ..] = the mode of each (-1 behind the last).  Always the
 * context's complete table.  Synchronous; returns 0, or the library's status codes. */
int eth_kzg_amd_test_fixed_msm_ex(const DASContext *ctx, int table_kind, int mode, int scalar_form, const uint8_t *scalars, int n_slices,
                                  uint8_t *out, int32_t *modes);

/* The scalars the prover hands to its fixed-base MSMs.  compute_cells_and_kzg_proofs' own schedule on n blobs (host, 1 <= n <= 4096,
 * both outputs asked for), then what it left for eth_kzg_amd_test_fixed_msm's stage, word for word: scalars[seg][blob][j < 128][i < 64][8]
 * little-endian words, each scalar as its two balanced GLV halves (sign in bit 127 of a half); seg < 4 for one or two blobs, < 2 for
 * three or four (copies scaled by 2^32, 2^64, 2^96 / by 2^64), one otherwise.  *n_words = words written (<= max_words, else 3).
 * cells[n][128][2048], proofs[n][128][48], status[n] (0, or 1: an element >= r): the call's outputs.  *fused_launches = launches of
 * k_coeffs_to_cells_scalars by this call: 1 where the scalars came from the cells' transform, 0 where k_fk20_scalars wrote them
 * (ETH_KZG_AMD_FUSED_SCALARS = 0 | 1 forces either at every batch size).  Synchronous. */
int eth_kzg_amd_test_prover_scalars(const DASContext *ctx, int n, const uint8_t *blobs, uint32_t *scalars, uint64_t max_words,
                                    uint64_t *n_words, uint8_t *cells, uint8_t *proofs, int32_t *status, int32_t *fused_launches);

/* The prover's G1 stage on its own: from the 128 sums per blob its fixed-base MSMs leave to the 128 proofs' bytes, by the launches
 * compute_cells_and_kzg_proofs makes behind the MSM (the engine's one statement of them) -- the compiled linear map (k_g1slp.hip) or, for
 * one or two blobs, the circulant form (k_g1circ.hip), then the compression.  n blobs (lanes), 1 <= n <= 256.  program: -1 = the engine's
 * own choice for n, 0 .. 5 = that compilation of the linear map at this n (refused with 3 where n takes the circulant form).
 * sums_words (host): raw words of the device's signed 13 x 30-bit Jacobian points (X, Y, Z: 13 words each), any digit pattern the type
 * admits.  Linear-map mode: [128][n]; slot j holds what the MSM leaves there, y_j / 2 in natural Fourier order.  Circulant mode:
 * [128][segs * n], segs = 4 for one or two blobs; lane seg * n + b holds 2^(128 seg / segs) u_j of blob b (u_j = y_j / 128), the scaled
 * copies the MSM produces from k_fk20_scalars' segment copies.  The padding lanes hold the identity.  out_proofs[n][128][48] (host).
 * Synchronous; returns 0, or the library's status codes.
 *
 * eth_kzg_amd_test_linmap_program: what the context uploaded for compilation `program`: words (4 per operation: dst slot, a slot, b,
 * flags -- csrc/g1_linmap.hpp: Schedule), launches[i] = (kind, first operation, count), *n_slots, consts[i] = constant i as canonical
 * big-endian bytes.  The counts come back in *n_words, *n_launches, *n_consts; a buffer that is too small: 3, with the counts set. */
int eth_kzg_amd_test_proofs_from_sums(const DASContext *ctx, int program, int n, const int32_t *sums_words, uint8_t *out_proofs);
int eth_kzg_amd_test_linmap_program(const DASContext *ctx, int program, uint32_t *words, uint64_t max_words, uint64_t *n_words,
                                    int32_t *launches, uint64_t max_launches, uint64_t *n_launches, int32_t *n_slots, uint8_t *consts,
                                    uint64_t max_consts, uint64_t *n_consts);

/* The many-message SHA-256 kernel (csrc/k_sha256.hip) on its own: n messages, message i = prefix[prefix_len] (HOST memory) |
 * (d_body + i * body_stride)[body_len] | (d_tail + i * tail_stride)[tail_len] (device memory; a part of length 0 may be NULL), digest i
 * -> d_out + 32 i (device).  Synchronous; returns 0 on success. */
int eth_kzg_amd_test_sha256_many(const DASContext *ctx, uint64_t n, const uint8_t *prefix, uint64_t prefix_len, const uint8_t *d_body,
                                 uint64_t body_stride, uint64_t body_len, const uint8_t *d_tail, uint64_t tail_stride, uint64_t tail_len,
                                 uint8_t *d_out);

/* The verifier's two-job bucket MSM on its own.  points: n_pts compressed G1 points (host); job 0 = sum_{i<n0} sc0[i] P_i, job 1 =
 * sum_{i<n1} sc1[i] P_i, 1 <= n0 <= n1 <= n_pts, scalars canonical big-endian < r (host).  out: the two sums, compressed (96 bytes).
 * form: 0 windowed (msm_pippenger2); 1 byte-shifted after pip_shift_prepare (one lane per point); 2 byte-shifted after
 * pip_shift_prepare_and_subgroup exactly as verify.hip launches it (quad form below coop_points_max, one-lane form above), with
 * status0/status1 over the first n0 / the remaining points; sub_status (n_pts ints, may be NULL) receives them (forms 0 and 1: the
 * status words of the production decompression, same values: 0 good, 1 bad encoding or off the curve, 2 outside the subgroup).
 * Synchronous.  Returns 0 on success, the library's status codes otherwise (a scalar >= r: 1; counts out of range: 3). */
int eth_kzg_amd_test_verify_msm(const DASContext *ctx, int form, const uint8_t *points, int n_pts, const uint8_t *sc0, int n0,
                                const uint8_t *sc1, int n1, uint8_t *out96, int32_t *sub_status);

/* What the batch verifiers hand to their pairing checks, as bytes (tests/test_verify_inputs.py compares them with an independent
 * statement in exact integers: the Fiat-Shamir challenge, its powers, the weights, the coset factors and the interpolation sums all
 * show in them; a verdict shows none of that for valid inputs).  Synchronous; return 0 on success, the library's status codes otherwise.
 *
 * eth_kzg_amd_test_verify_cells_partial_device: the device-resident form of eth_kzg_amd_verify_cell_kzg_proof_batch_partial -- the flat
 *   arrays of eth_kzg_amd_verify_cell_kzg_proof_batch_device (n >= 1 entries, device memory), the cells [lo, hi) evaluated under the
 *   challenge of the whole batch, out96 (host) = compress(sum r^k pi_k) | compress(the second pairing input).  It runs the set-up
 *   eth_kzg_amd_verify_cell_kzg_proof_batch_device runs: the pinned host mirror that arrives in chunks behind events, the device source.
 * eth_kzg_amd_test_verify_blob_batch_inputs: eth_kzg_verify_blob_kzg_proof_batch (on_device = 0: blobs / commitments / proofs are arrays
 *   of n host pointers) or eth_kzg_amd_verify_blob_kzg_proof_batch_device (on_device = 1: flat arrays in device memory), n >= 1, with the
 *   two sums the pairing check pairs handed out: out96 (host) = compress(sum r^i pi_i) | compress(sum r^i C_i - (sum r^i y_i) G +
 *   sum r^i z_i pi_i), paired with [tau]_2 and -[1]_2; *verified = the verdict of that check. */
int eth_kzg_amd_test_verify_cells_partial_device(const DASContext *ctx, uint64_t n, const uint8_t *d_commitments,
                                                 const uint64_t *d_cell_indices, const uint8_t *d_cells, const uint8_t *d_proofs, uint64_t lo,
                                                 uint64_t hi, uint8_t *out96);
int eth_kzg_amd_test_verify_blob_batch_inputs(const DASContext *ctx, uint64_t n, int on_device, const void *blobs, const void *commitments,
                                              const void *proofs, uint8_t *out96, int32_t *verified);

/* The leaf-hashed challenge of the cell verifier (c_eth_kzg.h: ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT; tests/test_gpu_leaf_transcript.py).
 * eth_kzg_amd_test_cell_leaf_digests: the leaf kernel (csrc/k_sha256.hip: k_sha256_cell_leaves) behind the staging and the launch of the
 *   flagged verification -- de-duplicated commitments, the row array, 32-bit indices, the arena's offsets.  Flat HOST arrays of n >= 1
 *   entries: commitments n * 48 bytes, cell_indices n uint64 (each below 128, else 3), cells n * 2048, proofs n * 48; any bytes will do
 *   (the call returns behind the digests, before a decoding verdict is read).  out_digests (host): n * 32 bytes, LEAF_0 .. LEAF_{n-1}.
 * eth_kzg_amd_test_verify_cells_inputs_ex: the whole batch through eth_kzg_amd_verify_cell_kzg_proof_batch_ex (on_device = 0:
 *   commitments / cells / proofs are arrays of n host pointers, cell_indices n uint64 on the host) or ..._device_ex (on_device = 1: the four
 *   flat arrays in device memory), n >= 1, flags as the public calls take them.  root32 (host) = the 32 digest bytes the challenge was
 *   reduced from (flags = 0: of the reference's transcript; leaf flag: ROOT), out96 (host) = compress(sum r^k pi_k) | compress(the second
 *   pairing input) over all n cells.
 * Synchronous; return 0 on success, the library's status codes otherwise (a NULL buffer or an unknown flag: 3). */
int eth_kzg_amd_test_cell_leaf_digests(const DASContext *ctx, uint64_t n, const uint8_t *commitments, const uint64_t *cell_indices,
                                       const uint8_t *cells, const uint8_t *proofs, uint8_t *out_digests);
int eth_kzg_amd_test_verify_cells_inputs_ex(const DASContext *ctx, uint64_t n, int on_device, const void *commitments,
                                            const void *cell_indices, const void *cells, const void *proofs, uint32_t flags, uint8_t *root32,
                                            uint8_t *out96);

/* ONE pass of eth_kzg_amd_verify_cell_kzg_proof_batch_many with what it pairs handed out (tests/test_verify_inputs.py compares every byte
 * with the statement of tests/verify_transcript.py: per-problem power tables, positions, row weights, sums, the folding weights, the fold
 * and the search's probes all show in them; a verdict shows none of that).  The arguments of the public call (host pointers), and exactly its
 * launches: the engine's pass fills a tap from the pinned read-backs it makes anyway, nothing is added on the device; points are compressed
 * on the host.  The hook serves one pass: a call the engine would cut -- into parts from 192 problems with 24576 cells, into chunks above
 * 131072 cells -- returns 3 before anything is launched, as does a NULL buffer (probe buffers may be NULL when max_probes is 0).
 *   verified[B], status[B]: as the public call gives them.
 *   form4: short-chain form (1 / 0), folded (1 / 0), the search ran (1 / 0), the folded check's verdict (1 / 0; -1 when not folded).
 *   sums96[B][96]: compress(A_b) | compress(B_b), the two sums of problem b that pair with [tau^64]_2 and -[1]_2; unspecified for a problem
 *     that is empty or whose status is not 0.
 *   rho[B][4]: the folding weights, little-endian words as uploaded (folded passes; 0 for a problem that takes no part).
 *   fold96: compress(S_0) | compress(S_1), S_j = sum_b rho_b sums[b][j] (folded passes).
 *   probe_ranges[i] = (lo, hi, passed), probe_sums96[i] = the pair summed over problems lo <= b < hi with the same weights: the probes of the
 *     search for the wrong problems, in the order they were made, the first max_probes of them; *n_probes = how many were made.
 * Synchronous; returns 0 on success, the library's status codes otherwise. */
int eth_kzg_amd_test_verify_many_sums(const DASContext *ctx, uint64_t n_batches, const uint64_t *commitments_lengths,
                                      const uint8_t *const *const *commitments, const uint64_t *cell_indices_lengths,
                                      const uint64_t *const *cell_indices, const uint64_t *cells_lengths, const uint8_t *const *const *cells,
                                      const uint64_t *proofs_lengths, const uint8_t *const *const *proofs, int32_t *verified, int32_t *status,
                                      int32_t *form4, uint8_t *sums96, uint32_t *rho, uint8_t *fold96, int32_t *probe_ranges,
                                      uint8_t *probe_sums96, uint64_t max_probes, uint64_t *n_probes);

/* The same pass over either source and with either challenge (c_eth_kzg.h: eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex /
 * _many_device_ex; tests/test_gpu_many_leaf.py, the statement is tests/many_leaf.py).  _ex: the pointer lists of the public call;
 * _device: flat arrays in device memory plus cell_starts (host, n_batches + 1 entries), as the public device form takes them, on the
 * context's first device.  flags: 0 or ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT.  Every output of eth_kzg_amd_test_verify_many_sums, and
 *   digests32[B][32]: the 32 bytes each problem's challenge was reduced from -- the reference transcript's digest, or the problem's
 *     ROOT under the flag; zero for a problem that was not hashed (empty, or refused at validation).  These are what the fold seed hashes.
 *   leaves32[N][32] (may be NULL; written under the flag only): LEAF_k of every cell in the caller's order, N = all cells of the call;
 *     zero for the cells of a problem that was refused at validation.
 * The same rules: one pass only (3 before any launch if the call would be cut, for a NULL buffer, an unknown flag or a malformed
 * cell_starts), and nothing is added on the device: the tap copies the read-backs the pass makes anyway. */
int eth_kzg_amd_test_verify_many_sums_ex(const DASContext *ctx, uint64_t n_batches, const uint64_t *commitments_lengths,
                                         const uint8_t *const *const *commitments, const uint64_t *cell_indices_lengths,
                                         const uint64_t *const *cell_indices, const uint64_t *cells_lengths, const uint8_t *const *const *cells,
                                         const uint64_t *proofs_lengths, const uint8_t *const *const *proofs, uint32_t flags, int32_t *verified,
                                         int32_t *status, int32_t *form4, uint8_t *sums96, uint32_t *rho, uint8_t *fold96, int32_t *probe_ranges,
                                         uint8_t *probe_sums96, uint64_t max_probes, uint64_t *n_probes, uint8_t *digests32, uint8_t *leaves32);
int eth_kzg_amd_test_verify_many_sums_device(const DASContext *ctx, uint64_t n_batches, const uint64_t *cell_starts, const uint8_t *d_commitments,
                                             const uint64_t *d_cell_indices, const uint8_t *d_cells, const uint8_t *d_proofs, uint32_t flags,
                                             int32_t *verified, int32_t *status, int32_t *form4, uint8_t *sums96, uint32_t *rho, uint8_t *fold96,
                                             int32_t *probe_ranges, uint8_t *probe_sums96, uint64_t max_probes, uint64_t *n_probes,
                                             uint8_t *digests32, uint8_t *leaves32);

/* The same tap on a pass of eth_kzg_amd_verify_data_columns / _device (c_eth_kzg.h; tests/test_gpu_data_columns.py, the expansion into
 * problems is tests/data_columns.py): problem b of every output above is column b.  on_device = 0: commitments / cells / proofs are the
 * host form's pointer lists; 1: the device form's flat arrays in device memory (context's first device).  And
 *   counts2[0]: the commitment points the pass handed to the decoding and subgroup-test launches (the unique commitments, once per pass)
 *   counts2[1]: the 255-bit products of decoded points the pass's launchers were given: n_columns * n_blobs proofs, n_columns *
 *               unique commitments and one h^64 * A per column (the interpolation commitments' fixed-base terms are not counted)
 *   Both are the HOST's launch arguments, not counters read back from the device: they follow the branch the pass took, so they tell a
 *   column pass from a forward to _many; that every product ran and ran once is what the byte-for-byte pairs say, not these.
 * One pass only (3 before any launch if the call would be cut, for a NULL buffer, an unknown flag or a column that validation refuses:
 * the outputs are indexed by column, and refused columns are taken out of the call before its passes); nothing is added on the device. */
int eth_kzg_amd_test_verify_data_columns_sums(const DASContext *ctx, uint64_t n_blobs, int on_device, const void *commitments,
                                              uint64_t n_columns, const uint64_t *column_indices, const void *cells, const void *proofs,
                                              uint32_t flags, int32_t *verified, int32_t *status, int32_t *form4, uint8_t *sums96, uint32_t *rho,
                                              uint8_t *fold96, int32_t *probe_ranges, uint8_t *probe_sums96, uint64_t max_probes,
                                              uint64_t *n_probes, uint8_t *digests32, uint8_t *leaves32, uint64_t *counts2);

/* The same tap on a pass of eth_kzg_amd_verify_partial_data_columns / _device (tests/test_gpu_partial_columns.py; the expansion into
 * problems is tests/partial_columns.py): the arguments of eth_kzg_amd_test_verify_data_columns_sums plus the bitmaps -- on_device = 0:
 * present is the host form's list of n_columns pointers, cells / proofs its pointer lists; 1: present is the flat [n_columns][W] array
 * (host), cells / proofs the packed device arrays.  Problem b of every output is column b, leaves32 holds the leaves of the present
 * cells column after column.  counts2[0]: the unique commitments of the call, decoded once per pass; counts2[1]: n proofs, one
 * product per (column, commitment) PAIR and one h^64 * A per column.  One pass only, and 3 for a column that validation refuses. */
int eth_kzg_amd_test_verify_partial_data_columns_sums(const DASContext *ctx, uint64_t n_blobs, int on_device, const void *commitments,
                                                      uint64_t n_columns, const uint64_t *column_indices, const void *present,
                                                      const void *cells, const void *proofs, uint32_t flags, int32_t *verified,
                                                      int32_t *status, int32_t *form4, uint8_t *sums96, uint32_t *rho, uint8_t *fold96,
                                                      int32_t *probe_ranges, uint8_t *probe_sums96, uint64_t max_probes,
                                                      uint64_t *n_probes, uint8_t *digests32, uint8_t *leaves32, uint64_t *counts2);

/* eth_kzg_amd_verify_kzg_proof_many / _many_device with a tap (csrc/point_many.hip; the statement is tests/point_many.py): exactly the
 * public call's launches, on the context's first device.  on_device = 0: commitments / zs / ys / proofs are the host form's pointer
 * lists; 1: the device form's flat arrays in device memory.  1 <= n <= 2^20.  forced_pass: 0 = the product's pass size, else the call is
 * cut into passes of that many items.  Outputs (host; the passes run one after the other so that they come in order):
 *   verified[n], status[n]: as the public call gives them.
 *   pass_starts[*n_passes + 1]: the first item of every pass, then n; returns 3 before any launch if there would be more than
 *     max_passes passes.
 *   leaves32[n][32], seeds32[passes][32], rho[n][4] (little-endian words as uploaded): LEAF_i, SEED and rho_i of every item / pass.
 *   fold96[passes]: compress(first sum) | compress(second sum) of the full-range pair of every pass; fold_verdicts[passes]: whether it
 *     passed the pairing check.
 *   probes4[i] = (pass, lo, hi, passed), lo <= position in the pass < hi, and probe_sums96[i] = that range's pair: the probes of the
 *     searches in the order they were made, the first max_probes of them; *n_probes = how many were made.
 * Synchronous; returns 0 on success, the library's status codes otherwise. */
int eth_kzg_amd_test_verify_kzg_proof_many_sums(const DASContext *ctx, uint64_t n, int on_device, const void *commitments, const void *zs,
                                                const void *ys, const void *proofs, uint64_t forced_pass, int32_t *verified, int32_t *status,
                                                uint64_t *pass_starts, uint64_t max_passes, uint64_t *n_passes, uint8_t *leaves32,
                                                uint8_t *seeds32, uint32_t *rho, uint8_t *fold96, int32_t *fold_verdicts, int32_t *probes4,
                                                uint8_t *probe_sums96, uint64_t max_probes, uint64_t *n_probes);

/* k_blob_eval_at alone (csrc/k_ntt.hip): y_b = p_b(z_b) for n blobs, 1 <= n <= 4096, on the context's first device.  blobs[b] -> 131072
 * bytes and zs_be32[n][32] (big-endian; a value >= r is reduced) on the host.  Outputs, host: out_ys_be32[n][32] canonical big-endian,
 * out_bad[n] = 1 for a blob that holds an element >= r (its y is 32 zero bytes).  Synchronous; 0 on success. */
int eth_kzg_amd_test_blob_eval_at(const DASContext *ctx, uint64_t n, const uint8_t *const *blobs, const uint8_t *zs_be32,
                                  uint8_t *out_ys_be32, int32_t *out_bad);

/* eth_kzg_amd_test_verify_kzg_proof_many_sums for the blob source (eth_kzg_amd_verify_blob_kzg_proof_many / _many_device): on_device = 0:
 * blobs / commitments / proofs are the host form's pointer lists; 1: the device form's flat arrays.  forced_pass: 0 = the product's pass
 * size of the blob source.  Every output as there, and zs32[n][32], ys32[n][32]: the z_i and y_i the passes computed, as their leaves
 * hash them (y_i = zero bytes for a refused blob). */
int eth_kzg_amd_test_verify_blob_kzg_proof_many_sums(const DASContext *ctx, uint64_t n, int on_device, const void *blobs,
                                                     const void *commitments, const void *proofs, uint64_t forced_pass, int32_t *verified,
                                                     int32_t *status, uint64_t *pass_starts, uint64_t max_passes, uint64_t *n_passes,
                                                     uint8_t *leaves32, uint8_t *seeds32, uint32_t *rho, uint8_t *fold96,
                                                     int32_t *fold_verdicts, int32_t *probes4, uint8_t *probe_sums96, uint64_t max_probes,
                                                     uint64_t *n_probes, uint8_t *zs32, uint8_t *ys32);

/* k_blob_to_extension alone (csrc/k_ntt.hip) behind the copy of cells 0..63: the extended blob of n blobs, 1 <= n <= 1024, on the
 * context's first device.  blobs[b] -> 131072 bytes on the host.  Outputs, host: out_cells[n][128][2048] -- cells 0..63 the blob's bytes,
 * cells 64..127 the kernel's (zero bytes for a refused blob) --, out_bad[n] = the problem's cell-status word: 1 for a blob that holds an
 * element >= r, else 0.  Synchronous; 0 on success. */
int eth_kzg_amd_test_blob_extension(const DASContext *ctx, uint64_t n, const uint8_t *const *blobs, uint8_t *out_cells, int32_t *out_bad);

/* k_blob_to_columns alone (csrc/k_ntt.hip; the kernel of eth_kzg_amd_blobs_to_data_columns): ONE launch over n blobs, 1 <= n <= 1024, that
 * are blobs [b0, b0 + n) of a column matrix of n_total blobs, b0 + n <= n_total <= 4096, on the context's first device.  blobs[b] -> 131072
 * bytes on the host.  matrix, host, [128][n_total][2048]: goes up as the caller filled it (a guard pattern), is written by the launch and
 * comes down again -- cell c of blob b at ((c * n_total + b0 + b) * 2048); a refused blob writes nothing.  blob_half = 0: rows 0..63 are
 * not written (the host form's launch).  out_bad[n] = the status words: 1 for a blob that holds an element >= r, else 0.  Synchronous;
 * 0 on success, 3 for a bad argument before anything is launched. */
int eth_kzg_amd_test_blob_to_columns(const DASContext *ctx, uint64_t n, const uint8_t *const *blobs, uint64_t n_total, uint64_t b0, int blob_half,
                                     uint8_t *matrix, int32_t *out_bad);

/* The tap of eth_kzg_amd_test_verify_many_sums_device on a pass of eth_kzg_amd_verify_blob_cell_proofs_many / _many_device (c_eth_kzg.h;
 * tests/test_gpu_blob_cells.py, the expansion into problems is tests/blob_cells.py): problem b of every output is item b, 128 cells each
 * (leaves32: n x 128 x 32 bytes).  on_device = 0: blobs / commitments / proofs are the host form's pointer lists; 1: the device form's
 * flat arrays in device memory (context's first device).  One pass only (3 before any launch if the call would be cut, or for a NULL
 * buffer); nothing is added on the device. */
int eth_kzg_amd_test_verify_blob_cell_proofs_sums(const DASContext *ctx, uint64_t n, int on_device, const void *blobs, const void *commitments,
                                                  const void *proofs, int32_t *verified, int32_t *status, int32_t *form4, uint8_t *sums96,
                                                  uint32_t *rho, uint8_t *fold96, int32_t *probe_ranges, uint8_t *probe_sums96,
                                                  uint64_t max_probes, uint64_t *n_probes, uint8_t *digests32, uint8_t *leaves32);

/* k_pairing_check alone (csrc/k_pairing.hip), next to the host's checks of the same pairs.  key: 0 = ([tau^64]_2, -[1]_2), the cell
 * verifier's pair of keys; 1 = ([tau]_2, -[1]_2), the point verifier's.  pairs: n x 2 x 48 bytes, compressed G1 (on the curve; no subgroup
 * test), 1 <= n <= 65536.  They are decompressed on the host and become the passes' Jacobian form.  rescale, a word of flags: bit 0 = every
 * point is multiplied through by a Z != 1 of its own (non-normalised inputs); bit 1 = the second slot of entry (rescale >> 8) is left at
 * the 0xff poison of the passes' result slots.  Outputs, host: out_gpu[n] the kernel's verdicts, out_host[n] the host threads' (1 / 0;
 * -1 for a poisoned entry); out_miller_gpu / out_miller_host (each may be NULL): n x 576 bytes, the Miller values before the final
 * exponentiation, as the words of the tower's Fp12 (the host's: the product of the two single Miller loops; 1 for a poisoned entry).
 * Synchronous; 0 on success, 3 where the context has no device route (a key at infinity). */
int eth_kzg_amd_test_pairing_check_many(const DASContext *ctx, int key, uint64_t n, const uint8_t *pairs, int rescale, int8_t *out_gpu,
                                        int8_t *out_host, uint8_t *out_miller_gpu, uint8_t *out_miller_host);

/* out4[0] = the probes of the last call through one of the *_many_sums hooks whose pairing ran on the GPU (counting the single-entry probes
 * at the end of a search, which the probe lists of the cell form do not hold), out4[1] = the probes in that call's list; out4[2], out4[3] =
 * nanoseconds the last eth_kzg_amd_test_pairing_check_many spent on the GPU route (launch, verdict bytes down, wait) and on the host
 * threads' checks.  Returns 0. */
int eth_kzg_amd_test_search_stats(const DASContext *ctx, uint64_t *out4);

/* The Reed-Solomon decoder of recovery on its own (Engine::rs_decode in recover.hip, exactly the launches recovery runs).  R >= 1 blobs; blob r has
 * n_cells[r] cells with ascending indices cell_indices[r][..] < 128, 64 <= n_cells[r] <= 128 (anything else: return 3, nothing is
 * launched).  flat_source = 0: cells[r][k] -> 2048 bytes (the list form of recover_cells_and_proofs_batch); 1: cells[r][0] -> the flat
 * 128 x 2048 bytes of the extended blob, absent cells holding junk (the device-resident form's source).  Outputs, host, canonical
 * big-endian, each may be NULL: status[R] (0, 1 non-canonical cell element, 4 inconsistent), deg[R], zp[R][65][32] (coefficients of Z',
 * ascending), zeval[R][128][32], zcinv[R][128][32] (cell order), coeffs[R][4096][32].  Synchronous. */
int eth_kzg_amd_test_rs_decode(const DASContext *ctx, int R, const uint64_t *n_cells, const uint64_t *const *cell_indices,
                               const uint8_t *const *const *cells, int flat_source, int32_t *status, int32_t *deg,
                               uint8_t *zp, uint8_t *zeval, uint8_t *zcinv, uint8_t *coeffs);

/* One field or point operation of the kernels per element (csrc/k_test_ops.hip), on the raw words of the device structs.
 * eth_kzg_amd_test_op_info: word counts per element of operation `op` (0, 1, ... until it returns -1), whether it exists on the
 * device only (the pair / quad forms, the tree folds) and its name.  eth_kzg_amd_test_op: n elements of in_words each in, n of
 * out_words each out; on_device = 0 runs the host pass of the same source (ctx may be NULL; an error for the device-only forms). */
int eth_kzg_amd_test_op_info(int op, int32_t *in_words, int32_t *out_words, int32_t *device_only, const char **name);
int eth_kzg_amd_test_op(const DASContext *ctx, int op, int n, const int32_t *in, int32_t *out, int on_device);

/* The window tables themselves.  A GLV table of nominal width c (launch.hpp): glv_windows(c) windows of mixed widths, two blocks per group
 * (lower / upper windows), inside a block [window][base][digit], entry (base i, digit d) of a window of `bits` bits at
 * (i << (bits - 1)) + d - 1, 1 <= d <= 2^(bits - 1), 96 bytes = 24 words each.
 * kind: 0 the FK20 table (128 groups of 64 bases), 1 the commitment table (64 groups of 64).  which: 0 the complete table the next MSM
 * launch would snapshot, 1 the wider table under construction next to it (its ready groups only), 2 the table a progressive start
 * began on, while it is alive.  All return 0 on success, non-zero if there is no such table or an argument is out of range.
 *
 * eth_kzg_amd_test_table_info: out8 = nominal width, groups, bases per group, state (0 under construction, 1 complete, 2 abandoned),
 *   ready groups, payload bytes (the entries: nothing else), groups per launch of the builder (they share its scratch), pieces;
 *   piece_first_block[k] (up to max_pieces; may be NULL) = the first block, 2 * group + upper, of piece k (a piece holds whole blocks).
 * eth_kzg_amd_test_table_audit: the exact audit (csrc/table_audit.hpp) of EVERY entry of the ready groups, on the GPU: *visited = entries
 *   visited, *n_findings = entries with a finding, findings = the first max_findings of them as (group, window, base, d, reasons), sorted;
 *   reasons: 1 encoding, 2 off the curve, 4 step T[d] != T[d-1] + T[1], 8 window link, 16 zero entry of a live row, 32 non-zero entry of
 *   an identity row, 64 first entry of window 0 is not the base.  *ms (may be NULL) = the kernel's time.
 * eth_kzg_amd_test_table_read: the stored words of entries d0 .. d0 + n - 1 of row (group, window, base) -> out[n][24].
 * eth_kzg_amd_test_table_audit_buffer: the same audit of a caller's table -- its blocks one after the other ([group][lower | upper]) --
 *   over bases[n_groups * nb] (96 bytes each: x, y as 12 little-endian words of the Montgomery form x 2^384 mod p; the identity is all
 *   zero).  on_device = 0 runs the host pass of the same source (ctx may be NULL). */
int eth_kzg_amd_test_table_info(const DASContext *ctx, int kind, int which, int64_t *out8, int32_t *piece_first_block, int max_pieces);
int eth_kzg_amd_test_table_audit(const DASContext *ctx, int kind, int which, uint64_t *visited, uint64_t *n_findings, int32_t *findings,
                                 int max_findings, double *ms);
int eth_kzg_amd_test_table_read(const DASContext *ctx, int kind, int which, int group, int window, int base, int d0, int n, uint32_t *out);
int eth_kzg_amd_test_table_audit_buffer(const DASContext *ctx, int c, int n_groups, int nb, const uint32_t *table, const uint8_t *bases,
                                        int on_device, uint64_t *visited, uint64_t *n_findings, int32_t *findings, int max_findings);

#ifdef __cplusplus
}
#endif
#endif /* C_ETH_KZG_TEST_HOOKS_H */
