// Host-callable launchers of the HIP kernels (one translation unit per kernel family so that
// hipcc compiles them in parallel).  Pointers are device pointers; element types are noted.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace kzg {
struct Fr8;    // 8 x u32, Montgomery (engine.hpp)
struct Fp12w;  // 12 x u32, Montgomery
namespace launch {

void init_attributes();  // opt in to 128 KiB dynamic LDS for the NTT kernels
// Load every code object of the library now (k_msm.hip).  HIP loads a translation unit's code object when one of its kernels
// is first launched, and that load allocates device memory: a caller whose first recovery / first wide-table MSM happens while
// the table builder thread sits in a hipMalloc (seconds, when the driver is still wiping memory another process freed) would
// wait for it -- kernel launches, copies and events themselves do not (tools/alloc_test/probe_stall.cpp).
void preload_code_objects();

// k_ntt.hip
// The three Fr stages of the prover compute in the unsaturated 9 x 29-bit form (fr29.hpp): w29 = the twiddle table in that
// form (8192 x 9 words, built on the host by ntt_twiddles29 from the saturated table); inputs / outputs keep the engine's
// stored forms (saturated Montgomery coefficients, plain-integer scalars, big-endian bytes).
constexpr size_t SIZEOF_FR29 = 36;
void ntt_twiddles29(const void* w8192_mont_host /*Fr[8192]*/, void* out_host /*8192 x 36 B*/);
void blob_to_coeffs(int n, const uint8_t* blobs, void* coeffs /*Fr*/, void* canon /*Fr or null*/, int* status,
                    const void* w29, const Fr8& n_inv, hipStream_t st);
// y_b = p_b(z_b) for n blobs, inside the CU (k_blob_eval_at): blobs 4-byte aligned, z_mont[n] Montgomery Fr (fr_from_be32's output);
// y_be32[n][32] canonical big-endian bytes (4-byte aligned), y_mont[n] Montgomery Fr, bad[n] = 1 for a blob with an element >= r (its
// y is zero in both forms).  Writes nothing else and needs no workspace.
void blob_eval_at(int n, const uint8_t* blobs, const void* z_mont, uint8_t* y_be32, void* y_mont, int* bad, const void* w29, const Fr8& n_inv,
                  hipStream_t st);
// cells 64..127 of n blobs, inside the CU (k_blob_to_extension): cells = [n][128][2048] bytes, 16-byte aligned, the first half of every
// slice holding its blob; the second half is written (zeros for a blob with an element >= r, whose status[b] gets bit 0 set; status[n]
// is not written otherwise).  Writes nothing else and needs no workspace.
void blob_to_extension(int n, uint8_t* cells, int* status, const void* w29, const Fr8& n_inv, hipStream_t st);
// The column layout of a block's data columns (eth_kzg_amd_compute_data_columns / _recover_data_columns): a launch over n blobs that are
// blobs [b0, b0 + n) of a call of n_total writes cell c of its blob b to cells + ((size_t)c * n_total + b0 + b) * 2048 and proof c to
// proofs + ((size_t)c * n_total + b0 + b) * 48, the output pointers being the WHOLE call's arrays.  Null: the blob-major layout
// [blob][128] from the pointer on, what every other call launches (its kernels are the instantiations they always were).
struct Columns {
    size_t n_total, b0;
};
void coeffs_to_cells(int n, const void* coeffs, uint8_t* cells, const void* w29, hipStream_t st, const Columns* cols = nullptr);
// eth_kzg_amd_blobs_to_data_columns: the three kernels that put what a caller with proofs in hand needs at its sidecar address.
// blob_to_columns (k_blob_to_columns): all 128 cells of n blobs (4-byte aligned, read where they lie) inside the CU, straight into the
// column matrix `cells` (4-byte aligned); blob_half = false leaves rows 0..63 alone; status (may be null) gets bit 0 set for a blob with
// an element >= r, which writes nothing.  cells_to_columns: the same matrix from n extended blobs [n][128][2048] (16-byte aligned).
// proofs_to_columns: proofs [n][128][48] -> out [128][n_total][48], both from any byte address.
void blob_to_columns(int n, const uint8_t* blobs, uint8_t* cells, const Columns& cols, bool blob_half, int* status, const void* w29, const Fr8& n_inv,
                     hipStream_t st);
void cells_to_columns(int n, const uint8_t* src, uint8_t* cells, const Columns& cols, hipStream_t st);
void proofs_to_columns(int n, const uint8_t* proofs, uint8_t* out, const Columns& cols, hipStream_t st);
// cells 0..63 only, blob-major: blobs = [n][131072], the bytes of the n blobs the coefficients belong to (checked recovery's out_blobs)
void coeffs_to_blobs(int n, const void* coeffs, uint8_t* blobs, const void* w29, hipStream_t st);
// every scalar leaves as its balanced GLV halves (what launch::glv_split would make of it)
void fk20_scalars(int n, const void* coeffs, void* scalars, const void* w29, const Fr8& inv128, int segs, const Fr8* seg_shifts,
                  hipStream_t st);
// coeffs_to_cells and fk20_scalars in one launch (k_coeffs_to_cells_scalars: the scalars are an intermediate of the cells' transform).
// tapk: one half (2 x 4096 x 36 B) of the table fk20_tap_consts builds for the scale fk20_scalars would have been given; blobs + status
// (both may be null): cells 0..63 of a blob with status 0 are copied from its bytes instead of being transformed back.
void fk20_tap_consts(const void* w29, const Fr8& scale, void* out /*8192 x 36 B*/, hipStream_t st);
void coeffs_to_cells_scalars(int n, const void* coeffs, uint8_t* cells, void* scalars, const uint8_t* blobs, const int* status, const void* w29,
                             const void* tapk, int segs, const Fr8* seg_shifts, hipStream_t st, const Columns* cols = nullptr);
void test_ntt4096(const uint8_t* in, uint8_t* out, const void* w29, const Fr8& n_inv, int inverse_dit, hipStream_t st);
void test_scalars_be(const uint8_t* in, void* out, size_t n, hipStream_t st);
void test_field_mul(const uint8_t* a, const uint8_t* b, uint8_t* out, int n, int is_fp, hipStream_t st);
// k_test_ops.hip (hooks library only): one field or point operation per element on raw words; the HD operations also on the host
int test_op_info(int op, int* in_words, int* out_words, int* device_only, const char** name);
int test_op_host(int op, int n, const int32_t* in, int32_t* out);
int test_op_device(int op, int n, const int32_t* d_in, int32_t* d_out, hipStream_t st);
// k_table_audit.hip (hooks library only): table_audit.hpp over every entry of the groups [0, n_groups) behind `blocks` (two pointers
// per group), bases = their n_groups x nb G1Affine.  Device: out = a device audit::Out (visited count, findings).  Host: the same source.
constexpr int TABLE_FINDING_WORDS = 5;  // group, window, base, d, reasons (audit::R_*)
constexpr size_t SIZEOF_AUDIT_OUT = 24;
void table_audit_device(const void* const* blocks, const void* bases, int c, int n_groups, int nb, void* out, hipStream_t st);
void table_audit_host(const void* const* blocks, const void* bases, int c, int n_groups, int nb, unsigned long long* visited,
                      unsigned long long* n_findings, int32_t* findings, int max_findings);

// k_msm.hip
// A window table as the kernels see it: a device array of block pointers -- two per group (blocks[2 group + upper]: the lower
// ceil(W / 2) windows, the upper rest; inside a block [window][base][digit]) -- and the range [g0, g0 + gcnt) of groups this launch covers (of the n_groups MSMs per slice the scalars hold).
// Tables are allocated in pieces and published group by group while they are built (engine.hip: SharedTable): a launch over
// the groups already built on the new table and one over the rest on the old table make one MSM stage.
struct TabBlocks {
    const void* const* blocks;
    int g0, gcnt;
};
// GLV tables (packed 96-B entries, W = glv_windows(c) windows of c bits over the 128-bit half scalars; k_msm_glv.inc, one
// translation unit per width): mode 0 flat, 1 windowed, 2 four chunks per MSM.  The scalars must be stored as balanced GLV
// halves (glv_split, or k_fk20_scalars' fused split).  Entries and sums are in the signed 13 x 30-bit field (curve30.hpp).
// A GLV table is NAMED by its nominal width c and has W = ceil(128 / c) windows -- but W windows of c bits cover W c >= 128 bits, and
// at widths that do not divide 128 the surplus doubles the table for nothing (nine windows of 15 bits = 135 bits: 116 GB; the same
// nine windows as two of 15 and seven of 14 bits = 128 bits: 58 GB, the same 18 gathered additions).  So the windows have MIXED
// widths (round 5): b = floor(128 / W) bits, the lowest 128 - W b of them one bit more.  c = 16 and c = 8 divide 128: unchanged.
constexpr int glv_windows(int c) { return (128 + c - 1) / c; }
constexpr int glv_lower_windows(int c) { return (glv_windows(c) + 1) / 2; }  // windows in the lower block of a group
constexpr int glv_base_bits(int c) { return 128 / glv_windows(c); }
constexpr int glv_wide_windows(int c) { return 128 - glv_windows(c) * glv_base_bits(c); }  // the lowest windows, one bit wider
constexpr int glv_window_bits(int c, int w) { return glv_base_bits(c) + (w < glv_wide_windows(c) ? 1 : 0); }
constexpr int glv_window_lo(int c, int w) { return w * glv_base_bits(c) + (w < glv_wide_windows(c) ? w : glv_wide_windows(c)); }  // its first bit
// entries per base of the windows [w0, w1): sum of 2^(bits - 1)
constexpr size_t glv_entries_per_base(int c, int w0, int w1) {
    size_t n = 0;
    for (int w = w0; w < w1; w++) n += (size_t)1 << (glv_window_bits(c, w) - 1);
    return n;
}
constexpr int GLV_WIDTHS[] = {16, 15, 14, 12, 8};  // widest first: the order the engine tries them in
bool glv_width_supported(int c);
void glv_split(void* scalars, size_t n, hipStream_t st);
// The prover, recovery and the commitments keep their points in the signed 13 x 30-bit form (JacS, 156 B) from the MSM sums through the
// linear map's arena, the circulant form and the commitment's fold to the compression: their launchers take JacS and nothing else.
// Set-up, verification and the stage hooks compute in the 14 x 29-bit form (JacQ, 168 B).  The three launchers both sides share --
// msm_glv, g1_set_inf, g1_compress -- are told the format of their point array (FMT_*) at every call.
constexpr int FMT_JACQ = 0, FMT_JACS = 1;
void msm_glv(int c, int mode, const void* scalars, const TabBlocks& table, void* out /*JacQ or JacS by out_fmt*/, int n_groups, int n_slices, int nb, int out_stride,
             int brp_bits, const Fp12w& beta, hipStream_t st, int out_fmt);
// k_table.hip
#ifdef TABS_STRIDE_128
constexpr size_t SIZEOF_TABP = 128;   // EXPERIMENT: a GLV table entry on a line of its own (curve30.hpp)
#else
constexpr size_t SIZEOF_TABP = 96;    // a packed GLV table entry
#endif
size_t table_glv_entries(int c, int n_groups, int nb);
size_t table_glv_side_bytes(int c, int n_groups, int nb);
// scratch: 168 B per entry of the chunk; side: table_glv_side_bytes; false if the width is not built in.
// blocks: device array of 2 * n_groups block pointers of THIS chunk's groups (lower / upper windows of each)
bool build_table_glv(int c, const void* bases, void* const* blocks, void* scratch, void* side, int n_groups, int nb, int* err, hipStream_t st);

// k_g1fft.hip
void g1_fft_layer(void* X, int stride, int half, int tw_step, int inverse, int mode, const void* tw, const Fp12w& beta,
                  hipStream_t st);

// k_g1slp.hip: one launch of the straight-line program of the FK20 proofs map (g1_linmap.hpp) on an arena of JacS; kind = linmap::OpKind
void g1_slp_launch(int kind, void* arena, int stride, const uint32_t* words, int count, const void* naf, const Fp12w& beta,
                   hipStream_t st, int lanes = 0 /* lanes to run (a multiple of 64, from the arena pointer on); 0: all `stride` of them */,
                   int coop_lanes = 0 /* > 0: the batch has this many blobs (<= 64): the constant multiplications take four (<= 16) or two lanes per blob */,
                   int n_active = 0 /* blobs that are really there (0: all `lanes`): the padding lanes behind them are skipped */);

// k_g1misc.hip
void g1_set_inf(void* X, size_t n, hipStream_t st, int fmt);
int coop_points_max();  // largest launch (points) that takes the four-lanes-per-point kernels (k_g1misc.hip)
void spin(uint64_t wall_clock_ticks, hipStream_t st);  // one wave, resident for that many ticks of the constant-rate device clock
// cols (JacS only): the record of (position, slice) goes to out + ((size_t)pos * n_total + b0 + slice) * 48 instead of (slice * n_pos + pos) * 48
void g1_compress(const void* X, uint8_t* out, int n_pos, int stride, int n_slices, hipStream_t st, int fmt, const Columns* cols = nullptr);
void g1_sum_positions(void* X /*JacS*/, int n_pos, int stride, int n_slices, hipStream_t st);
// subgroup_check: 0 none, 1 endomorphism test, 2 definitional [r]P == O
void g1_decompress(const uint8_t* in, void* out /*G1Affine*/, int* status, int n, int subgroup_check, const Fp12w& beta,
                   hipStream_t st);
// two segments in one launch, production checks (on curve + subgroup)
void g1_decompress2(const uint8_t* in0, void* out0, int* status0, int n0, const uint8_t* in1, void* out1, int* status1, int n1,
                    const Fp12w& beta, hipStream_t st);
// its two halves as separate launches: decode + on-curve test (status 0 / 1), then the subgroup test of the decoded points (0 -> 0 / 2)
void g1_decode2(const uint8_t* in0, void* out0, int* status0, int n0, const uint8_t* in1, void* out1, int* status1, int n1,
                const Fp12w& beta, hipStream_t st);
void g1_subgroup2(const void* pts0, int* status0, int n0, const void* pts1, int* status1, int n1, const Fp12w& beta, hipStream_t st);
void fk20_srs_vectors(const void* srs, void* X, hipStream_t st);
void fk20_gather_bases(const void* X, void* bases, hipStream_t st);
void test_load_points(const uint8_t* in, void* X, int n_lanes, int stride, hipStream_t st);
void test_recompress(const void* pts, uint8_t* out, int n, hipStream_t st);

// twiddle recoding shared by engine.hip (host) and k_g1fft.hip (device)
constexpr int TWIDDLE_WNAF_W = 5;   // window width of the non-adjacent form (table of 2^(w-2) odd multiples)
constexpr int TWIDDLE_WORDS = 33;   // 132 signed digit bytes per 128-bit half
// k_g1circ.hip
constexpr int CIRC_LANES = 256;
size_t g1_circ_table_bytes(int n, int T);
void g1_circ128(void* X /*JacS*/, int stride, int n, int segs, void* D, int T, const void* terms, int per_lane, const Fp12w& beta, hipStream_t st);
// k_verify.hip
void init_attributes_verify();
// slot_of: destination cell slot per input cell (null = identity); status_of: status word per input cell (null = word 0)
void cells_to_fr(const uint8_t* cells, void* evals, const int* slot_of, int* status, const int* status_of, const int* src_of, int n,
                 hipStream_t st);
void rec_vanishing_poly(const uint32_t* present, const void* w8192, void* zp, int* deg, int R, hipStream_t st);
void rec_vanishing(const void* zp, const int* deg, const void* w8192, const Fr8& seven64, void* zeval, void* zcinv, int R,
                   hipStream_t st);
void verify_scalars(const Fr8* pow_table24, int k0, const int* cell_idx, const void* w8192, void* rp_mont, void* s1, void* s2,
                    int n, hipStream_t st);
void verify_weights(const void* rp_mont, const int* row, void* weights, int n, int m, hipStream_t st);
void interp(const void* evals, const int* cell_idx, const void* rp_mont, const void* w8192, const Fr8& inv64, void* partial,
            int nblocks, void* out_neg_canon, int n, hipStream_t st);
void interp_cells(const void* evals, const int* cell_idx, const void* w8192, const Fr8& inv64, void* coef, int n, hipStream_t st);
void interp_sum(const void* coef, const void* rp_mont, void* partial, int nblocks, void* out_neg_canon, int n, hipStream_t st);
// large verification batches: byte-shifted point copies built before the challenge is known (k_verify.hip)
size_t pip_shift_workspace_bytes(int n_max);
void pip_shift_prepare(const void* points, int n_pts, int n_max, void* workspace, const Fp12w& beta, hipStream_t st);
// the same and, in the same launch, the subgroup tests of two point segments (status 0 -> 0 / 2): one stream per verification
void pip_shift_prepare_and_subgroup(const void* points, int n_pts, int n_max, void* workspace, const void* pts0, int* status0, int n0,
                                    const void* pts1, int* status1, int n1, const Fp12w& beta, hipStream_t st);
void msm_pippenger2_shifted(const void* sc0, int n0, const void* sc1, int n1, int n_max, void* workspace, void* out_jacq2,
                            hipStream_t st);  // out: two JacQ (SIZEOF_JACQ each)
size_t pip_workspace_bytes(int n_max);
void copy_affine(const void* src, void* dst, int n, hipStream_t st);
void msm_pippenger2(const void* points, const void* sc0, int n0, const void* sc1, int n1, void* workspace, void* out_affine2,
                    const Fp12w& beta, hipStream_t st);
// fac_stride: factors per blob (128), or 0 when all R blobs share the 128 factors of one vanishing polynomial
void rec_dit_half(int R, const void* V, const void* fac, void* T, const void* w8192, hipStream_t st, int fac_stride = 128);
// canon (final pass only, may be null): the coefficients once more as canonical integers, what the commitment MSM reads
void rec_dit_last(int R, const void* T, const void* shift, const Fr8& n_inv, void* U, void* coeffs, int* status,
                  const void* w8192, int final_pass, hipStream_t st, void* canon = nullptr);
// checked recovery: status[b] |= REC_COMMITMENT_BIT where calc[48 b ..] differs from expected[48 b ..] (expected: any byte address)
constexpr int REC_COMMITMENT_BIT = 8;
void commitment_check(const uint8_t* calc, const uint8_t* expected, int* status, int n, hipStream_t st);
void rec_dif_half(int R, const void* U, const void* fac, void* V, const void* w8192, hipStream_t st, int fac_stride = 128);

// k_verify_many.hip: many independent verifications in one pass (per-problem scalars, one lane or quad per scalar multiplication).
// pts = [proofs n | commitments m] (G1Affine).  The expanded source has m rows over all problems (row_batch, row_start) and two scalars
// per proof; the column source (eth_kzg_amd_verify_data_columns: problem b = column b) has ONE list of m commitments, row[k] < m
// pass-wide, and one h_(c_b)^64 per column.  A launcher tells the column source by the pointer it names as null there.
// rp_mont[k] / s1[k] = r_b^k (Montgomery / canonical);  s2[k] = r_b^k h_k^64 (null: columns);  h64[b] canonical, 1 for a column
// without cells (null: expanded)
// Partial columns (eth_kzg_amd_verify_partial_data_columns): a column holds the blobs of its bitmap only, so its weights and w C products
// go by a sparse pair list where the dense column pass addresses (b, u) at b m + u: column b's pairs are start[b] .. start[b + 1], pair r
// is the commitment u[r] of the pass's list; count = start[n_batches] <= n.  start null: no pair list (every other source).
struct VmPairs { const int* start = nullptr; const int* u = nullptr; int count = 0; };
void vm_scalars(const void* pow_tables /*[B][24] Fr*/, const int* batch_of, const int* pos_in_batch, const int* cell_idx, const int* cell_start,
                const void* w8192, void* rp_mont, void* s1, void* s2, void* h64, int n, int n_batches, hipStream_t st);
// weights[m], or [n_batches][m] for columns (row_batch null), or one per pair
void vm_weights(const void* rp_mont, const int* row, const int* row_batch, const int* cell_start, void* weights, int m, int n_batches, hipStream_t st,
                const VmPairs& pairs = {});
void vm_interp_sum(const void* coef, const void* rp_mont, const int* cell_start, void* out_neg_canon, int n_batches, hipStream_t st);
// every scalar multiplication of the pass in ONE launch.  prod (JacQ): s1[e] pi_e n | s2[e] pi_e n | w[j] C_j m, or for columns (s2 null)
// s1[e] pi_e n | w[b][u] C_u n_batches m (pairs: w[r] C_(u[r]), count of them);  small (short-chain passes): behind them the 64 interpolation terms isc[b][j] SRS_j per
// problem, and the launch also holds the subgroup tests of the n + m points (status: 0 -> 0 / 2).  -> products of decoded points
int vm_products(const void* pts, const void* s1, const void* s2, const void* wts, const void* isc, const void* srs, void* prod, int n, int m,
                int n_batches, bool small, int* status, const Fp12w& beta, hipStream_t st, const VmPairs& pairs = {});
// out[b][2] JacQ: the two sums of problem b's products + (icommit ? icommit[b] : its 64 interpolation terms).  Columns (row_start null):
// out[2b + 1] = h64[b] out[2b] + the rest, a second launch of n_batches products behind the reduction (prod holds n_batches more
// JacQ behind the products).  -> products launched
int vm_sums(const void* prod, const void* icommit, const int* cell_start, const int* row_start, const void* h64, void* out /*[B][2] JacQ*/, int n,
            int m, int n_batches, const Fp12w& beta, hipStream_t st, const VmPairs& pairs = {});
// out2[j] = sum_b rho_b sums[b][j] (rho: 4 words per problem, 0 excludes it); prod: scratch of 2 B JacQ
void vm_fold(const void* sums, const uint32_t* rho, void* prod, void* out2, int n_batches, const Fp12w& beta, hipStream_t st);
// out[r][2] = the weighted pairs summed over problems ranges[r][0] .. ranges[r][1] - 1 (prod as vm_fold left it)
void vm_fold_ranges(const void* prod, const int* ranges /*[n_ranges][2], device*/, void* out /*[n_ranges][2] JacQ*/, int n_ranges, hipStream_t st);

// k_pairing.hip: verdict[i] = e(pairs[i][0], key0) e(pairs[i][1], key1) == 1 ? 1 : 0, or -1 where a pair still holds the 0xff poison of
// the result slots; pairs [n][2] JacQ, key0 / key1 68 prepared lines each (192 B), frob the three Frobenius constants (288 B), all in
// HBM.  miller (test hook; null in the product): [n] x 576 B, the Miller values before the final exponentiation
void pairing_check(const void* pairs, const void* key0, const void* key1, const void* frob, int8_t* verdict, int n, hipStream_t st,
                   void* miller = nullptr);

// k_point_many.hip: many verify_kzg_proof items in one pass (point_many.hip), one lane per scalar multiplication
// bodies[n][176] = "RCKZGPROOFLEAF_1" | commitment | z | y | proof per item, for sha256_many; all five arrays 4-byte aligned
void pm_leaf_bodies(const uint8_t* commitments, const uint8_t* zs, const uint8_t* ys, const uint8_t* proofs, uint8_t* bodies, int n, hipStream_t st);
// status[i] = 2 if point_status[n + i] (commitment) or point_status[i] (proof), else 1 if z_bad[i] or y_bad[i], else 0
void pm_status(const int* point_status /*[proofs n | commitments n]*/, const int* z_bad, const int* y_bad, int* status, int n, hipStream_t st);
// the blob source (verify_host.hpp: blob_item_status): status[i] = 1 if blob_bad[i], else 2 if point_status[n + i] or point_status[i], else 0
void pm_blob_status(const int* point_status /*[proofs n | commitments n]*/, const int* blob_bad, int* status, int n, hipStream_t st);
// pts = [proofs n | commitments n] (G1Affine), gen = G (G1Affine), z / y Montgomery Fr, rho[n][4].  pairs[2 i] = rho_i pi_i;
// terms[3][n] = rho C | (rho z) pi | (rho y) G; an item whose status is not 0 gets the identity everywhere (JacQ)
void pm_mul(const void* pts, const void* gen, const void* z_mont, const void* y_mont, const uint32_t* rho, const int* status, void* pairs, void* terms,
            int n, const Fp12w& beta, hipStream_t st);
// pairs[2 i + 1] = terms[0][i] + terms[1][i] - terms[2][i], exact
void pm_pairs(const void* terms, void* pairs, int n, hipStream_t st);

// k_4844.hip
void quotient_by_linear(int n, const void* coeffs, const void* z_mont, void* quotient, void* y_out, hipStream_t st);
// n x 32 big-endian bytes -> Montgomery Fr.  reduce: the value mod r (a digest becomes a challenge; bad is not touched); otherwise a
// value >= r gives bad[i] = 1 and the point 0
void fr_from_be32(int n, const uint8_t* in, void* out_mont, int* bad, bool reduce, hipStream_t st);
void fr_to_be32(int n, const void* canon /*Fr*/, uint8_t* out, hipStream_t st);
void fr_mont_to_be32(int n, const void* mont /*Fr*/, uint8_t* out, hipStream_t st);  // the same from the Montgomery form
// out[i] = 1 if blob_bad[i], else 1 if z_bad[i], else 2 if g1_bad[i], else 0 (z_bad / g1_bad may be null)
void status_4844(int n, const int* blob_bad, const int* z_bad, const int* g1_bad, int* out, hipStream_t st);

// k_sha256.hip: SHA-256 of n independent messages, one lane each; message i = prefix[prefix_len] | (body + i * body_stride)[body_len] |
// (tail + i * tail_stride)[tail_len], all device pointers (a part of length 0 may be null); digest i -> out + 32 i
void sha256_many(int n, const uint8_t* prefix, uint32_t prefix_len, const uint8_t* body, size_t body_stride, uint32_t body_len,
                 const uint8_t* tail, size_t tail_stride, uint32_t tail_len, uint8_t* out, hipStream_t st);
// the n leaves of the cell verifier's leaf-hashed challenge (verify_host.hpp: CellLeafTranscript), one lane each, from the verifier's
// arena: leaf k hashes k, idx[k], uniq + 48 row[k], proofs + 48 k and cells + 2048 k; digest k -> out + 32 k.  uniq, proofs and cells
// 16-byte aligned, out 32-byte aligned (anything else throws before the launch).  pos (the many-verification's arena: the cells of
// several problems back to back): leaf k hashes pos[k], its position inside its problem, in the place of k -- a second instantiation
// of the kernel; null: the single verification's
void sha256_cell_leaves(int n, const uint8_t* uniq, const int* row, const int* idx, const uint8_t* proofs, const uint8_t* cells, uint8_t* out,
                        hipStream_t st, const int* pos = nullptr);

constexpr size_t SIZEOF_FR = 32, SIZEOF_G1AFFINE = 96, SIZEOF_G1JAC = 144;
constexpr size_t SIZEOF_JACS = 156;  // signed 13 x 30-bit Jacobian point (curve30.hpp)
constexpr size_t SIZEOF_AFFQ = 112, SIZEOF_JACQ = 168;  // unsaturated 14 x 29-bit forms (curve29.hpp): affine points, FFT arrays

}  // namespace launch
}  // namespace kzg
