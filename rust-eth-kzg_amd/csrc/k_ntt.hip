// Fr kernels: blob decode + 4096-point NTT in LDS, cell encoding, FK20 circulant-column NTTs.
// Reference functions replaced: a1 deserialize, a2 bit reversal, a3 Fr NTT,
// a9 Toeplitz/circulant column FFTs, a11 cell serialisation.
#include "engine.hpp"
#include "kcommon.hpp"
#include "fr29.hpp"
#include "fr29_ntt.hpp"
#include "glv.hpp"
#include "launch.hpp"

namespace kzg {

// ------------------------------------------------------------------------------------------------
// LDS-resident 4096-point NTT in the unsaturated 9 x 29-bit form (fr29.hpp).  Layout: lds[limb * 4096 + index] (limb-major: a
// wave touching consecutive indices touches consecutive banks); 9 limbs = 144 KiB of the CU's 160 KiB.
// Both networks are Cooley-Tukey -- multiply the second input by the twiddle, then add / subtract -- so a value's bound
// grows by 2 r per layer and nothing is reduced inside a transform (bounds at every call site).
__device__ __forceinline__ Fr29 lds_load(const uint32_t* s, int idx) {
    Fr29 r;
#pragma unroll
    for (int l = 0; l < RL; l++) r.v[l] = s[l * N_BLOB + idx];
    return r;
}
__device__ __forceinline__ void lds_store(uint32_t* s, int idx, const Fr29& a) {
#pragma unroll
    for (int l = 0; l < RL; l++) s[l * N_BLOB + idx] = a.v[l];
}

// w29[k] = omega_8192^k in the 9 x 29-bit Montgomery form (canonical), k < 8192.  omega_m^j = w29[j * 8192/m].
//
// RADIX-4 PASSES IN REGISTERS (round 5).  Two layers of the radix-2 network are one pass: a thread loads the four
// elements i0 + {0, h, 2h, 3h} of a unit, runs the two butterflies of the first layer and the two of the second on them in registers,
// and stores four results -- the same four products as before (in a prime field the fourth root of unity is a twiddle like any other:
// radix 4 saves no multiplication), but half the LDS round trips, half the index arithmetic, and the first layer's sums and
// differences stay un-swept (fr29.hpp, LAZY LIMBS: they are what the second layer reads).  Bit-identical to the radix-2 network.
// Thread tid owns unit tid (1024 units of four elements).  Which passes need a block barrier follows from who wrote a unit's
// elements in the pass before (worked out at the two functions): three barriers per transform instead of six.
struct LdsElems {  // the transform's 4096 elements in LDS, limb-major (lds_load / lds_store above)
    uint32_t* s;
    __device__ __forceinline__ Fr29 load(int i) const { return lds_load(s, i); }
    __device__ __forceinline__ void store(int i, const Fr29& v) const { lds_store(s, i, v); }
};
// Inverse transform: input in bit-reversed order -> natural order, inverse twiddles omega^-j, in LDS, 1024 threads.
// Bound: in < B  ->  out < B + 24.
// Pass h (layers half = h, then 2h): unit u = blk * h + j (j < h) holds the elements blk * 4h + j + {0, h, 2h, 3h}; they were written
// in pass h / 4 by the units (4 blk + k) * (h / 4) + (j mod h / 4), k < 4: the same 4-, 16-, 64-thread group for h = 4, 16, 64 (a wave's
// LDS operations execute in program order: no barrier), four different waves for h = 256 and h = 1024 (a block barrier before each).
// The last pass leaves unit j's results at j + 1024 k -- exactly what thread j reads afterwards: no barrier at the end.
__device__ __forceinline__ void dit_inverse_pass(uint32_t* s, const Fr29* __restrict__ w29, int h) {
    ntt4096_dit_inverse_unit(LdsElems{s}, w29, h, (int)threadIdx.x);
}
__device__ __forceinline__ void ntt4096_dit_inverse(uint32_t* s, const Fr29* __restrict__ w29) {  // the caller's barrier stands before
    dit_inverse_pass(s, w29, 1);
    __builtin_amdgcn_wave_barrier();
    dit_inverse_pass(s, w29, 4);
    __builtin_amdgcn_wave_barrier();
    dit_inverse_pass(s, w29, 16);
    __builtin_amdgcn_wave_barrier();
    dit_inverse_pass(s, w29, 64);
    __syncthreads();
    dit_inverse_pass(s, w29, 256);
    __syncthreads();
    dit_inverse_pass(s, w29, 1024);
    __builtin_amdgcn_wave_barrier();  // thread j reads j + 1024 k next: its own unit's results
}
// Forward transform: natural order -> bit-reversed order (position q holds X[brp(q)]), Cooley-Tukey butterflies with the
// twiddles taken in bit-reversed order: at stride `half` the block i = q / half uses omega_4096^(brp(i) * half).
// (Round 2 used Gentleman-Sande butterflies here, whose sum path doubles the bound per layer.)  Bound: in < B -> out < B + 24.
// Pass h (layers half = 2h, then h; log_m = log2(1024 / h) blocks of 4h elements): unit u = blk * h + j holds blk * 4h + j + {0, h, 2h, 3h}.
// The first pass (h = 1024) reads j + 1024 k: what thread j itself stored in the input stage (no barrier before it); the passes h = 256
// and h = 64 read other waves' results (a block barrier before each); h = 16, 4, 1 stay inside the 64-thread group that wrote their
// elements; the callers read across waves afterwards: a block barrier at the end.
__device__ __forceinline__ void ct_forward_pass(uint32_t* s, const Fr29* __restrict__ w29, int h, int log_m) {
    ntt4096_ct_forward_unit(LdsElems{s}, w29, h, log_m, (int)threadIdx.x);
}
// The transform in two parts, so that k_coeffs_to_cells_scalars can read the FK20 scalars between them (fr29_ntt.hpp, THE FK20 TAP).
// After the head, thread tid's own stores of pass h = 64 are the elements (tid / 64) * 256 + (tid mod 64) + {0, 64, 128, 192}: the tap
// reads exactly those, what the same thread wrote, so it needs NO barrier of its own (a wave's LDS operations execute in program
// order), and it writes nothing to LDS: the wave barrier in front of the tail stands as it did between the passes h = 64 and h = 16.
__device__ __forceinline__ void ntt4096_ct_forward_head(uint32_t* s, const Fr29* __restrict__ w29) {  // input stored by thread e mod 1024
    __builtin_amdgcn_wave_barrier();
    ct_forward_pass(s, w29, 1024, 0);
    __syncthreads();
    ct_forward_pass(s, w29, 256, 2);
    __syncthreads();
    ct_forward_pass(s, w29, 64, 4);
}
__device__ __forceinline__ void ntt4096_ct_forward_tail(uint32_t* s, const Fr29* __restrict__ w29) {
    __builtin_amdgcn_wave_barrier();
    ct_forward_pass(s, w29, 16, 6);
    __builtin_amdgcn_wave_barrier();
    ct_forward_pass(s, w29, 4, 8);
    __builtin_amdgcn_wave_barrier();
    ct_forward_pass(s, w29, 1, 10);
    __syncthreads();
}
__device__ __forceinline__ void ntt4096_ct_forward(uint32_t* s, const Fr29* __restrict__ w29) {
    ntt4096_ct_forward_head(s, w29);
    ntt4096_ct_forward_tail(s, w29);
}
__device__ __forceinline__ Fr fr_words_of(const Fr29& canonical) {
    Fr r;
    fr29_to_words(r.v, canonical);
    return r;
}
// An MSM scalar leaves as its balanced GLV halves k = k1 + k2 lambda (glv.hpp), the form the window tables' kernels extract their
// digits from.  x: the plain value, < 2r, normalised limbs.
__device__ __forceinline__ void store_split_scalar(Fr* __restrict__ at, const Fr29& x) {
    Fr k = fr_words_of(fr29_reduce_once(x));
    uint32_t h[8];
    glv_split_balanced(k, h);
#pragma unroll
    for (int l = 0; l < 8; l++) k.v[l] = h[l];
    *at = k;
}

// Stage A+B of compute_cells_and_kzg_proofs: blob bytes -> monomial coefficients.
//   coeffs = IFFT_4096(bit_reverse(blob))   (fk20/prover.rs:177-180, domain.rs:199-211)
// The inverse network wants its input bit-reversed, i.e. exactly the blob as given: no permutation pass.
// grid = n_blobs, block = 1024, dynamic LDS = 144 KiB.  status[b] |= 1 if any element >= r.
// Outputs stay in the engine's stored forms: coeffs = saturated Montgomery (8 x 32 bits, canonical), canon_out = the
// plain integers (MSM scalars), both through the final multiplication by n^-1 with the right constant.
// The blob's elements go through the inverse transform as the PLAIN integers they are (round 5): a product of a plain value with a
// twiddle in Montgomery form is plain again, so the conversion product the input stage had (x * 2^522 / 2^261) is gone, and the
// final product every element has anyway carries the 2^261 instead.
struct NttConsts {
    Fr29 ninv_to_sat;   // n^-1 * 2^256 * 2^261 mod r: mul(x, .) = x n^-1 2^256 = the saturated Montgomery form of the coefficient
    Fr29 ninv_plain;    // n^-1 * 2^261 mod r: mul(x, .) = x n^-1
    Fr29 one;           // 2^261 mod r: mul(x, .) = x (the test kernel's forward direction: reduction only)
};
__global__ __launch_bounds__(1024) void k_blob_to_coeffs(const uint8_t* __restrict__ blobs, Fr* __restrict__ coeffs,
                                                        Fr* __restrict__ canon_out, int* __restrict__ status,
                                                        const Fr29* __restrict__ w29, NttConsts K) {
    extern __shared__ uint32_t s[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint8_t* blob = blobs + (size_t)b * BYTES_PER_BLOB;
    bool bad = false;
    for (int e = tid; e < N_BLOB; e += 1024) {
        const Fr x = load_fr_be(blob + 32 * e);
        bad |= geq_mod<FrParams>(x.v);
        lds_store(s, e, fr29_from_plain(x));  // the integer itself: < 2^256 < 3r, normalised limbs
    }
    if (bad) atomicOr(&status[b], 1);
    __syncthreads();
    ntt4096_dit_inverse(s, w29);  // < 27 r
    for (int e = tid; e < N_BLOB; e += 1024) {
        const Fr29 x = lds_load(s, e);
        coeffs[(size_t)b * N_BLOB + e] = fr_words_of(fr29_reduce_once(fr29_mul(x, K.ninv_to_sat)));
        if (canon_out) canon_out[(size_t)b * N_BLOB + e] = fr_words_of(fr29_reduce_once(fr29_mul(x, K.ninv_plain)));
    }
}

// y = p(z) of a blob at one point WITHOUT LEAVING THE CU (the blob source of the point many-verification, point_many.hip): the input
// stage and the inverse transform of k_blob_to_coeffs, then the evaluation of the 4096 coefficients where they lie -- no coefficient and
// no quotient goes to HBM (the verifiers' other road, k_blob_to_coeffs + k_quotient_by_linear, writes 128 KB of each per blob and needs
// the engine's workspace; this kernel owns none).  grid = n_blobs, block = 1024, dynamic LDS = 144 KiB; plus 2.8 KB static.
//   z_mont[b]   the point in the saturated Montgomery form (what k_fr_from_be32 writes)
//   y_be32[b]   y as 32 big-endian canonical bytes;  y_mont[b]  y in the saturated Montgomery form (what k_pm_mul reads)
//   bad[b]      1 if the blob holds an element >= r: then y is zero in both forms and nothing is transformed
// After the transform thread j holds the UNSCALED coefficients c_(j + 1024 k) = n a_(j + 1024 k), k < 4, as plain integers (its own unit's
// results), and  n p(z) = sum_j z^j (c_j + z^1024 (c_(j+1024) + z^1024 (c_(j+2048) + z^1024 c_(j+3072)))).
// Powers (Montgomery form, x 2^261, every one a fresh product: < 2r, limbs normalised): wave 0 builds the tables z^a (lanes 0..31) and
// z^(32 b) (lanes 32..63) with one branch-free square-and-multiply, 5 + 10 products a lane; then per thread z^1024 = z^(32 31) z^32 and
// z^j = z^(j mod 32) z^(32 (j / 32)): 2 products, 3 for the Horner steps, 1 for z^j: at most 21 products on any thread, 6 on most.
// A plain value times a Montgomery-form power is plain again, so the block sum S = n p(z) (plain) leaves through ONE product per output
// form with the constants k_blob_to_coeffs applies per coefficient: S ninv_plain = y, S ninv_to_sat = y 2^256.
__device__ __forceinline__ Fr29 fr29_shfl_xor(const Fr29& a, int mask) {
    Fr29 r;
#pragma unroll
    for (int l = 0; l < RL; l++) r.v[l] = __shfl_xor(a.v[l], mask);
    return r;
}
// sum over the 8 lanes that differ in the bits `first`, 2 first, 4 first: in < 2r with limbs < 2^29 -> < 4r (limbs < 2^30), < 8r (< 2^31),
// < 16r (8 (2^29 - 1) < 2^32: no limb wraps) -> swept and brought back below 2r (16r < 2^261: fr29_partial_reduce's range)
__device__ __forceinline__ Fr29 fr29_sum8_lanes(Fr29 a, int first) {
    a = fr29_add<false>(a, fr29_shfl_xor(a, first));      // < 4r
    a = fr29_add<false>(a, fr29_shfl_xor(a, 2 * first));  // < 8r
    a = fr29_add<false>(a, fr29_shfl_xor(a, 4 * first));  // < 16r: the headroom of the limbs ends here
    return fr29_partial_reduce(a);                        // < 2r, limbs normalised
}
__global__ __launch_bounds__(1024) void k_blob_eval_at(const uint8_t* __restrict__ blobs, const Fr* __restrict__ z_mont,
                                                      uint8_t* __restrict__ y_be32, Fr* __restrict__ y_mont, int* __restrict__ bad_out,
                                                      const Fr29* __restrict__ w29, NttConsts K) {
    extern __shared__ uint32_t s[];
    __shared__ uint32_t pw[2][RL][32];  // [0]: z^a, [1]: z^(32 b); limb-major like s
    __shared__ uint32_t wave_sum[RL][16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint8_t* blob = blobs + (size_t)b * BYTES_PER_BLOB;
    bool bad = false;
    for (int e = tid; e < N_BLOB; e += 1024) {
        const Fr x = load_fr_be(blob + 32 * e);
        bad |= geq_mod<FrParams>(x.v);
        lds_store(s, e, fr29_from_plain(x));  // the integer itself: < 2^256 < 3r, normalised limbs
    }
    if (tid < 64) {  // wave 0, no divergence: lanes 0..31 raise z, lanes 32..63 raise z^32, to the power tid mod 32
        const bool hi = tid >= 32;
        Fr29 base = fr29_partial_reduce(fr29_from_fr_mont(z_mont[b]));  // z 2^261: < 32r -> < 2r
#pragma unroll 1
        for (int i = 0; i < 5; i++) {
            const Fr29 sq = fr29_mul(base, base);
#pragma unroll
            for (int l = 0; l < RL; l++) base.v[l] = hi ? sq.v[l] : base.v[l];
        }
        Fr29 acc = K.one;  // 2^261 mod r: the Montgomery form of 1
#pragma unroll 1
        for (int bit = 4; bit >= 0; bit--) {
            acc = fr29_mul(acc, acc);
            const Fr29 m = fr29_mul(acc, base);
            const bool take = ((tid & 31) >> bit) & 1;
#pragma unroll
            for (int l = 0; l < RL; l++) acc.v[l] = take ? m.v[l] : acc.v[l];
        }
#pragma unroll
        for (int l = 0; l < RL; l++) pw[hi ? 1 : 0][l][tid & 31] = acc.v[l];
    }
    const bool refused = __syncthreads_or(bad) != 0;  // the barrier between the input stage (and the tables) and what reads them
    if (refused) {                                    // uniform over the block
        if (tid < 8) {
            reinterpret_cast<uint32_t*>(y_be32 + (size_t)b * 32)[tid] = 0;
            y_mont[b].v[tid] = 0;
        }
        if (tid == 0) bad_out[b] = 1;
        return;
    }
    ntt4096_dit_inverse(s, w29);  // < 27 r; thread tid's own unit left tid + 1024 k
    auto power = [&](int t, int e) {
        Fr29 r;
#pragma unroll
        for (int l = 0; l < RL; l++) r.v[l] = pw[t][l][e];
        return r;
    };
    const Fr29 z1024 = fr29_mul(power(1, 31), power(1, 1));
    Fr29 acc = lds_load(s, tid + 3072);                                         // < 27r
    acc = fr29_add<false>(fr29_mul(acc, z1024), lds_load(s, tid + 2048));       // 27 x 2 <= 64: < 2r, + < 27r: < 29r, limbs < 2^30
    acc = fr29_add<false>(fr29_mul(acc, z1024), lds_load(s, tid + 1024));       // 29 x 2 <= 64: < 29r again
    acc = fr29_add<false>(fr29_mul(acc, z1024), lds_load(s, tid));              // < 29r
    Fr29 t = fr29_mul(acc, fr29_mul(power(0, tid & 31), power(1, tid >> 5)));   // 29 x 2 <= 64: this thread's share of n p(z), < 2r
    // the block sum: 1024 values < 2r are 2048r, far beyond 2^261 ~ 70r: reduced after every three levels (fr29_sum8_lanes)
    t = fr29_sum8_lanes(t, 1);
    t = fr29_sum8_lanes(t, 8);  // the wave's 64: < 2r
    if ((tid & 63) == 0) {
#pragma unroll
        for (int l = 0; l < RL; l++) wave_sum[l][tid >> 6] = t.v[l];
    }
    __syncthreads();
    if (tid >= 64) return;
    const int w = tid & 15;  // wave 0: every lane takes part in the shuffles, lanes 16.. hold copies
#pragma unroll
    for (int l = 0; l < RL; l++) t.v[l] = wave_sum[l][w];
    t = fr29_sum8_lanes(t, 1);                       // 8 waves: < 2r
    t = fr29_add<false>(t, fr29_shfl_xor(t, 8));     // all 16: S = n p(z) mod r, < 4r, limbs < 2^30
    if (tid == 0) {
        store_fr_be(y_be32 + (size_t)b * 32, fr_words_of(fr29_reduce_once(fr29_mul(t, K.ninv_plain))));  // 4 x 1 <= 64
        y_mont[b] = fr_words_of(fr29_reduce_once(fr29_mul(t, K.ninv_to_sat)));
        bad_out[b] = 0;
    }
}

// Cells 64..127 of a blob WITHOUT LEAVING THE CU (the blob source of the cell many-verification, verify_many.hip): the input stage and
// the inverse transform of k_blob_to_coeffs, the twist by w8192^e and the forward transform of half 1 of k_coeffs_to_cells, on one LDS
// image -- no coefficient goes to HBM and the kernel owns no workspace.  grid = n_blobs, block = 1024, dynamic LDS = 144 KiB (one block
// per CU, as every transform of this file).
//   cells     [n][128][2048]: the slice of blob b holds the blob's bytes in its first half (cells 0..63 ARE the blob: copied by the
//             caller, never transformed back); this kernel writes the second half, each Fr once, big-endian, at its final address
//   status[b] |= 1 if the blob holds an element >= r (the word k_cells_to_fr sets for the same problem): nothing is transformed then
//             and the second half is written as zeros, so that whoever hashes or decodes the slice reads nothing stale
// Values.  The blob's elements are plain integers (< 2^256 < 3r); after the inverse transform (< 27r) thread j holds the UNSCALED
// coefficients c_e = n a_e, e = j + 1024 k, plain.  x_e = c_e w8192^e is one product against w29 (27 x 1 <= 64: < 2r, plain again, limbs
// normalised: the forward network's input bound with room to spare); the forward network leaves n X[2 q' + 1] bit-reversed in place
// (< 2 + 24 = 26r), and the n^-1 the coefficients never got rides on the product every output has anyway: 26 x 1 <= 64, K.ninv_plain
// where k_coeffs_to_cells multiplies by one.  No premultiplied table: it would save nothing over w29.
// Barriers.  The inverse network's last pass leaves unit j's results at j + 1024 k, and the forward network's first pass (h = 1024) reads
// j + 1024 k: both are thread j's own unit (comments at the two networks), so the twist in between, which loads and stores exactly
// those four elements, needs no barrier of its own: a wave's LDS operations execute in program order.
__global__ __launch_bounds__(1024) void k_blob_to_extension(uint8_t* __restrict__ cells, int* __restrict__ status,
                                                           const Fr29* __restrict__ w29, NttConsts K) {
    extern __shared__ uint32_t s[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint8_t* blob = cells + (size_t)b * 2 * BYTES_PER_BLOB;
    uint8_t* ext = cells + ((size_t)b * 2 + 1) * BYTES_PER_BLOB;
    bool bad = false;
    for (int e = tid; e < N_BLOB; e += 1024) {
        const Fr x = load_fr_be(blob + 32 * e);
        bad |= geq_mod<FrParams>(x.v);
        lds_store(s, e, fr29_from_plain(x));  // the integer itself: < 2^256 < 3r, normalised limbs
    }
    const bool refused = __syncthreads_or(bad) != 0;  // the barrier between the input stage and the transform
    if (refused) {                                    // uniform over the block
        for (int k = tid; k < BYTES_PER_BLOB / 16; k += 1024) reinterpret_cast<uint4*>(ext)[k] = make_uint4(0, 0, 0, 0);
        if (tid == 0) atomicOr(&status[b], 1);
        return;
    }
    ntt4096_dit_inverse(s, w29);  // < 27 r; thread tid's own unit left tid + 1024 k
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const int e = tid + 1024 * k;
        lds_store(s, e, fr29_mul(lds_load(s, e), w29[e]));  // 27 x 1 <= 64: n a_e w8192^e, < 2r
    }
    ntt4096_ct_forward(s, w29);  // < 26 r; its first pass reads what this thread has just stored
    for (int e = tid; e < N_BLOB; e += 1024)
        store_fr_be(ext + 32 * e, fr_words_of(fr29_reduce_once(fr29_mul(lds_load(s, e), K.ninv_plain))));  // 26 x 1 <= 64: X n / n = the value
}

// Stage H+I: cells = bit_reverse(NTT_8192(coeffs || 0)) serialised big-endian
// (prover.rs:158-165, serialization/src/lib.rs:132-156).  X[2k+h] = NTT_4096(a_i * w8192^(i*h))[k];
// the forward network leaves half h bit-reversed in place, which is exactly cells[h*4096 ...].
// grid = (n_blobs, 2), block = 1024, dynamic LDS = 144 KiB.
// Where the two cell writers below put element e of half h of blob b (cell 64 h + e / 64, element e % 64 of it).  Each Fr is stored
// once, from LDS to its final address, so the layout of the output is this address and nothing else:
//   CellsByBlob    [blob][128][2048]: the extended blob, what every call but the column forms launches
//   CellsByColumn  [128][n_total][2048], this launch's blob b being blob b0 + b of the call: the layout of a block's data column
//                  sidecars (eth_kzg_amd_compute_data_columns / _recover_data_columns).  128 n_total 2048 bytes pass 2^32: size_t throughout.
//   BlobsOnly      [blob][131072]: cells 0..63 and nothing else, which are the blob's own bytes (eth_kzg_amd_recover_data_columns_checked's
//                  out_blobs).  Launched with ONE block per blob (grid (n, 1)): half 1, the cells 64..127, is not computed at all.
struct CellsByBlob {
    uint8_t* cells;
    __device__ __forceinline__ uint8_t* fr(int b, int h, int e) const { return cells + ((size_t)b * N_EXT + (size_t)h * N_BLOB + e) * 32; }
};
struct CellsByColumn {
    uint8_t* cells;
    size_t n_total, b0;
    __device__ __forceinline__ uint8_t* fr(int b, int h, int e) const {
        return cells + (((size_t)(h * (N_CELLS / 2) + (e >> 6)) * n_total + b0 + b) * CELL_LEN + (e & (CELL_LEN - 1))) * 32;
    }
};
struct BlobsOnly {
    uint8_t* blobs;
    __device__ __forceinline__ uint8_t* fr(int b, int, int e) const { return blobs + ((size_t)b * N_BLOB + e) * 32; }
};
// All 128 cells of a blob at their SIDECAR addresses WITHOUT LEAVING THE CU (eth_kzg_amd_blobs_to_data_columns: the caller holds the
// proofs already, so nothing of FK20 runs): k_blob_to_extension's image, transforms, barriers and value bounds (comments there), read
// from the caller's blobs where they lie and written through CellsByColumn -- no coefficient goes to HBM, no workspace, no [blob][128]
// intermediate.  grid = n_blobs, block = 1024, dynamic LDS = 144 KiB.
//   kBlobHalf   the input stage also stores cells 0..63, which ARE the four elements a thread has just loaded: they wait in registers for
//               the verdict on the blob and leave before the transform starts.  false (the host form, whose helper threads copy that
//               half from the caller's own bytes): rows 0..63 of the matrix are not touched
//   status      (may be null) status[b] |= 1 if the blob holds an element >= r.  Such a blob writes NOTHING: its slots keep what they held
// Every output byte is written once: element e of half h at dst.fr(b, h, e), 32 bytes, 4-byte aligned like the blob.
template <bool kBlobHalf>
__global__ __launch_bounds__(1024) void k_blob_to_columns(const uint8_t* __restrict__ blobs, CellsByColumn dst, int* __restrict__ status,
                                                         const Fr29* __restrict__ w29, NttConsts K) {
    extern __shared__ uint32_t s[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint8_t* blob = blobs + (size_t)b * BYTES_PER_BLOB;
    Fr own[4];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int e = tid + 1024 * k;
        own[k] = load_fr_be(blob + 32 * e);
        bad |= geq_mod<FrParams>(own[k].v);
        lds_store(s, e, fr29_from_plain(own[k]));  // the integer itself: < 2^256 < 3r, normalised limbs
    }
    const bool refused = __syncthreads_or(bad) != 0;  // the barrier between the input stage and the transform
    if (refused) {                                    // uniform over the block
        if (tid == 0 && status) atomicOr(&status[b], 1);
        return;
    }
    if (!dst.cells) return;  // a caller that wants the status words alone (uniform over the grid)
    if (kBlobHalf) {
#pragma unroll
        for (int k = 0; k < 4; k++) store_fr_be(dst.fr(b, 0, tid + 1024 * k), own[k]);  // the bytes as they came: any 256-bit value round-trips
    }
    ntt4096_dit_inverse(s, w29);  // < 27 r; thread tid's own unit left tid + 1024 k
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const int e = tid + 1024 * k;
        lds_store(s, e, fr29_mul(lds_load(s, e), w29[e]));  // 27 x 1 <= 64: n a_e w8192^e, < 2r
    }
    ntt4096_ct_forward(s, w29);  // < 26 r; its first pass reads what this thread has just stored
    for (int e = tid; e < N_BLOB; e += 1024)
        store_fr_be(dst.fr(b, 1, e), fr_words_of(fr29_reduce_once(fr29_mul(lds_load(s, e), K.ninv_plain))));  // 26 x 1 <= 64: X n / n = the value
}
// The flagged form of the same call (verify_many.hip): the pass has every blob's 128 cells in its arena, blob-major, for the leaves and
// the decoding; this copies them to their sidecar addresses behind the extension step.  src [n][128][2048], 16-byte aligned (the
// arena's); grid = (n, 128), block = 128: a block moves one cell, a thread 16 bytes of it; vec16: the matrix is 16-byte aligned too
// (it is 4-byte aligned always, like the output of k_blob_to_columns).
__global__ __launch_bounds__(128) void k_cells_to_columns(const uint8_t* __restrict__ src, CellsByColumn dst, int vec16) {
    const int b = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
    const uint4 v = *reinterpret_cast<const uint4*>(src + ((size_t)b * N_CELLS + c) * BYTES_PER_CELL + 16 * t);
    uint8_t* to = dst.fr(b, c >> 6, (c & 63) << 6) + 16 * t;  // element 0 of cell c
    if (vec16) {
        *reinterpret_cast<uint4*>(to) = v;
    } else {
        uint32_t* w = reinterpret_cast<uint32_t*>(to);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
}
// The proofs a caller holds per blob, [n][128][48], to where the sidecars carry them: dst [128][n_total][48], blob b of this launch being
// blob b0 + b.  A plain re-ordering: the 48 bytes are never decoded.  T = uint32_t where both arrays are 4-byte aligned (a proof is 12
// words), else uint8_t: any byte address.  A thread moves one unit; units = n * 128 * 48 / sizeof(T).
template <class T>
__global__ __launch_bounds__(256) void k_proofs_to_columns(const T* __restrict__ src, T* __restrict__ dst, size_t n_total, size_t b0, size_t units) {
    constexpr size_t U = 48 / sizeof(T);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= units) return;
    const size_t p = i / U, j = i % U, b = p / N_CELLS, k = p % N_CELLS;
    dst[(k * n_total + b0 + b) * U + j] = src[i];
}

template <class Dst>
__global__ __launch_bounds__(1024) void k_coeffs_to_cells(const Fr* __restrict__ coeffs, Dst dst, const Fr29* __restrict__ w29) {
    extern __shared__ uint32_t s[];
    const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    for (int e = tid; e < N_BLOB; e += 1024) {
        Fr29 c = fr29_from_fr_mont(coeffs[(size_t)b * N_BLOB + e]);  // < 32 r
        if (h && e) c = fr29_mul(c, w29[e]);                          // < 2 r
        lds_store(s, e, c);
    }
    __syncthreads();
    ntt4096_ct_forward(s, w29);  // < 56 r
    const Fr29 one_plain = fr29_const(r29::ONE_PLAIN);
    for (int e = tid; e < N_BLOB; e += 1024)
        store_fr_be(dst.fr(b, h, e), fr_words_of(fr29_reduce_once(fr29_mul(lds_load(s, e), one_plain))));  // X / 2^261 = the value
}

// ------------------------------------------------------------------------------------------------
// Stage C: the 64 circulant-column NTT_128 of FK20 (h_poly.rs:36-56, toeplitz.rs:132-144,
// batch_toeplitz.rs:94-106).  For blob b and i < 64 the length-128 vector is
//   v[0] = a[4095-i];  v[1..64] = 0;  v[64+k] = a[64k-1-i], k = 1..63
// scalars[b][j][i] = NTT_128(v)[j] * 128^-1  (the 128^-1 of the later G1 inverse FFT, domain.rs:189-191,
// folded in here because everything downstream is linear), stored as balanced GLV halves (glv.hpp) for the MSM's window extraction.
// grid = n_blobs * 16, block = 256 (4 vectors per block, one per wave).
// segs > 1 (tiny batches only): copies of every scalar multiplied by 2^(128 seg / segs) are written as extra "blobs"
// seg * n + b, so that the MSM stage also delivers 2^32 u, 2^64 u, 2^96 u (four segments; 2^64 u for two) and the
// doubling chain of k_g1circ.hip splits into `segs` independent shorter chains.
struct SegShifts { Fr29 p[3]; };  // the segment shifts as plain integers times 2^261 (this form), p[seg - 1]
__global__ __launch_bounds__(256) void k_fk20_scalars(const Fr* __restrict__ coeffs, Fr* __restrict__ scalars,
                                                      const Fr29* __restrict__ w29, Fr29 scale /* 32 x (128^-1 or 1/2) as an integer: see the input stage */, int n,
                                                      int segs, SegShifts sh) {
    __shared__ uint32_t s[4][RL][128];
    const int b = blockIdx.x >> 4, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = ((blockIdx.x & 15) << 2) + wv;
    const Fr* a = coeffs + (size_t)b * N_BLOB;
    uint32_t(*sv)[128] = s[wv];
    {
        // element `lane` (0..63) and element 64+lane
        Fr29 lo, hi;
#pragma unroll
        for (int l = 0; l < RL; l++) lo.v[l] = hi.v[l] = 0;
        // The vectors go through the transform as PLAIN integers (round 5, as in k_blob_to_coeffs): the stored coefficient is the integer
        // Y = y 2^256, the product with the integer 32 s is Y 32 s / 2^261 = y s, a plain value times a Montgomery-form twiddle stays plain,
        // and the output needs a reduction below r instead of a Montgomery product by one.
        if (lane == 0) lo = fr29_mul(fr29_from_plain(a[N_BLOB - 1 - i]), scale);  // (< r) x (< r) -> < 2r
        else hi = fr29_mul(fr29_from_plain(a[64 * lane - 1 - i]), scale);
#pragma unroll
        for (int l = 0; l < RL; l++) { sv[l][lane] = lo.v[l]; sv[l][64 + lane] = hi.v[l]; }
    }
    __builtin_amdgcn_wave_barrier();
    // natural -> bit-reversed, Cooley-Tukey with bit-reversed twiddles (see ntt4096_ct_forward): < 2 + 14 = 16 r
    int log_m = 0;
    for (int half = 64; half >= 1; half >>= 1, log_m++) {
        const int j = lane & (half - 1), blk = lane / half;
        const int i0 = ((lane - j) << 1) + j, i1 = i0 + half;
        const int e = log_m ? (int)(__brev((unsigned)blk) >> (32 - log_m)) * half * (N_EXT / 128) : 0;  // omega_128 = omega_8192^64
        Fr29 x, y;
#pragma unroll
        for (int l = 0; l < RL; l++) { x.v[l] = sv[l][i0]; y.v[l] = sv[l][i1]; }
        const Fr29 t = e ? fr29_mul(y, w29[e]) : fr29_partial_reduce(y);
        Fr29 sum = fr29_add<false>(x, t), d = fr29_sub2r<false>(x, t);
        if ((log_m & 1) || half == 1) { fr29_normalise(sum); fr29_normalise(d); }  // every second layer and the last one sweep the carries (fr29.hpp, LAZY LIMBS)
#pragma unroll
        for (int l = 0; l < RL; l++) { sv[l][i0] = sum.v[l]; sv[l][i1] = d.v[l]; }
        __builtin_amdgcn_wave_barrier();  // a wave owns its whole vector: its LDS operations execute in program order, no block barrier
    }
    // position q holds NTT[brp7(q)].  The scalar leaves already split k = k1 + k2 lambda for the GLV window tables (what the separate
    // k_glv_split pass of round 2 did in place: 0.19 ms of reading and writing 0.5 GB at 2048 blobs)
    auto emit = [&](size_t at, const Fr29& x) {  // x: the plain value, < 16 r (or < 2r: a segment's product)
        store_split_scalar(&scalars[at], fr29_partial_reduce(x));
    };
    for (int q = lane; q < 128; q += 64) {
        Fr29 x;
#pragma unroll
        for (int l = 0; l < RL; l++) x.v[l] = sv[l][q];
        const int j = __brev((unsigned)q) >> 25;
        emit(((size_t)b * 128 + j) * 64 + i, x);
        for (int sg = 1; sg < segs; sg++)  // (x sh) is this form again
            emit(((size_t)(sg * n + b) * 128 + j) * 64 + i, fr29_mul(x, sh.p[sg - 1]));  // plain x times the Montgomery form of the shift: plain
    }
}

// Stages H+I and C in one launch: k_coeffs_to_cells that also emits the FK20 scalars of its half of the extended domain, read from
// the transform's LDS image after the third pass (fr29_ntt.hpp, THE FK20 TAP: block h holds every scalar with j = h mod 2 up to one
// constant factor; barriers: ntt4096_ct_forward_head).  Same grid, LDS layout and passes as k_coeffs_to_cells; the scalars' layout and
// form are k_fk20_scalars' (segment copies included), bit for bit.  tapk: launch::fk20_tap_consts for the wanted scale.
// Cells 0..63 are the blob (the transform of half 0 inverts k_blob_to_coeffs): with `blobs` given and blob b accepted (status 0: every
// element canonical, so its bytes ARE the canonical encoding), block h = 0 stops after its scalars and copies the 128 KiB across.  A
// rejected blob, and a caller without the blob's bytes (blobs = null), finish the transform.
template <class Dst>
__global__ __launch_bounds__(1024) void k_coeffs_to_cells_scalars(const Fr* __restrict__ coeffs, Dst dst,
                                                                 Fr* __restrict__ scalars, const uint8_t* __restrict__ blobs,
                                                                 const int* __restrict__ status, const Fr29* __restrict__ w29,
                                                                 const Fr29* __restrict__ tapk, int n, int segs, SegShifts sh) {
    extern __shared__ uint32_t s[];
    const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    for (int e = tid; e < N_BLOB; e += 1024) {
        Fr29 c = fr29_from_fr_mont(coeffs[(size_t)b * N_BLOB + e]);  // < 32 r
        if (h && e) c = fr29_mul(c, w29[e]);                          // < 2 r
        lds_store(s, e, c);
    }
    __syncthreads();
    ntt4096_ct_forward_head(s, w29);  // < 32 + 12 = 44 r
    const int e0 = ((tid >> 6) << 8) + (tid & 63);  // this thread's unit of pass h = 64
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const int e = e0 + 64 * k;
        const Fr29 x = fk20_tap_scalar(LdsElems{s}, tapk, e, h);  // (< 44 r) x (< r): the plain scalar, < 2r
        const size_t at = (size_t)fk20_tap_row(e, h) * 64 + fk20_tap_column(e);
        store_split_scalar(&scalars[(size_t)b * N_EXT + at], x);
        for (int sg = 1; sg < segs; sg++)  // plain x times the Montgomery form of the shift: plain (k_fk20_scalars)
            store_split_scalar(&scalars[(size_t)(sg * n + b) * N_EXT + at], fr29_mul(x, sh.p[sg - 1]));
    }
    if (h == 0 && blobs && status[b] == 0) {  // uniform over the block: no barrier follows
        const uint4* src = reinterpret_cast<const uint4*>(blobs + (size_t)b * BYTES_PER_BLOB);
        for (int k = tid; k < BYTES_PER_BLOB / 16; k += 1024)  // 16 bytes = half an element: element k / 2 of half 0
            *reinterpret_cast<uint4*>(dst.fr(b, 0, k >> 1) + 16 * (k & 1)) = src[k];
        return;
    }
    ntt4096_ct_forward_tail(s, w29);  // < 56 r
    const Fr29 one_plain = fr29_const(r29::ONE_PLAIN);
    for (int e = tid; e < N_BLOB; e += 1024)
        store_fr_be(dst.fr(b, h, e), fr_words_of(fr29_reduce_once(fr29_mul(lds_load(s, e), one_plain))));  // X / 2^261 = the value
}
__global__ void k_fk20_tap_consts(const Fr29* __restrict__ w29, Fr29 scale_plain, Fr29* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < 2 * N_BLOB) out[idx] = fk20_tap_const(w29, scale_plain, idx);
}

#ifdef KZG_TEST_HOOKS  // stage-level test kernels: compiled into libc_eth_kzg_hooks.so only (csrc/Makefile)
__global__ __launch_bounds__(1024) void k_test_ntt4096(const uint8_t* in, uint8_t* out, const Fr29* w29, NttConsts K, int inverse_dit) {
    extern __shared__ uint32_t s[];
    for (int e = threadIdx.x; e < N_BLOB; e += 1024) lds_store(s, e, fr29_from_plain(load_fr_be(in + 32 * e)));  // plain values (see NttConsts)
    __syncthreads();
    if (inverse_dit) ntt4096_dit_inverse(s, w29);
    else ntt4096_ct_forward(s, w29);
    for (int e = threadIdx.x; e < N_BLOB; e += 1024) {
        const Fr29 c = lds_load(s, e);
        store_fr_be(out + 32 * e, fr_words_of(fr29_reduce_once(fr29_mul(c, inverse_dit ? K.ninv_plain : K.one))));
    }
}
__global__ void k_test_scalars_be(const uint8_t* in, Fr* out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = load_fr_be(in + 32 * i);
}
template <class F>
__global__ void k_test_field_mul(const uint8_t* a, const uint8_t* b, uint8_t* out, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int NB = F::N * 4;
    F x, y;
    for (int k = 0; k < F::N; k++) {
        const uint8_t* pa = a + (size_t)i * NB + 4 * k;
        const uint8_t* pb = b + (size_t)i * NB + 4 * k;
        x.v[F::N - 1 - k] = ((uint32_t)pa[0] << 24) | ((uint32_t)pa[1] << 16) | ((uint32_t)pa[2] << 8) | pa[3];
        y.v[F::N - 1 - k] = ((uint32_t)pb[0] << 24) | ((uint32_t)pb[1] << 16) | ((uint32_t)pb[2] << 8) | pb[3];
    }
    F z = from_mont(mul(to_mont(x), to_mont(y)));
    for (int k = 0; k < F::N; k++) {
        uint32_t w = z.v[F::N - 1 - k];
        uint8_t* po = out + (size_t)i * NB + 4 * k;
        po[0] = (uint8_t)(w >> 24); po[1] = (uint8_t)(w >> 16); po[2] = (uint8_t)(w >> 8); po[3] = (uint8_t)w;
    }
}

#endif

namespace launch {
// the code object of this translation unit is loaded now (HIP loads a code object on the first launch of one of its kernels, and
// that load is an allocation: it would wait behind a table piece the builder thread is allocating)
void preload_k_ntt() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_blob_to_coeffs));
}
static Fr as_fr(const Fr8& x) { Fr r; for (int i = 0; i < 8; i++) r.v[i] = x.v[i]; return r; }

constexpr size_t LDS_NTT29 = (size_t)N_BLOB * RL * 4;  // 144 KiB: one 4096-point transform of 9-limb elements resident in LDS
void init_attributes() {
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_blob_to_coeffs), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_NTT29);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_blob_eval_at), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_NTT29);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_blob_to_extension), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_NTT29);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_blob_to_columns<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_NTT29);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_blob_to_columns<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_NTT29);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_coeffs_to_cells<CellsByBlob>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_NTT29);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_coeffs_to_cells<CellsByColumn>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_NTT29);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_coeffs_to_cells<BlobsOnly>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_NTT29);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_coeffs_to_cells_scalars<CellsByBlob>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_NTT29);
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_coeffs_to_cells_scalars<CellsByColumn>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_NTT29);
#ifdef KZG_TEST_HOOKS
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_test_ntt4096), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_NTT29);
#endif
}
// host-side constants of the 9 x 29-bit form from the engine's saturated Montgomery values (Y = y 2^256 mod r, canonical)
// X = y 2^261 mod r = 32 Y mod r: in Fr arithmetic, the Montgomery form of (y * 32) read as a plain integer
static Fr29 fr29_mont_of(const Fr& y_mont) {
    Fr c32 = zero<FrParams>();
    c32.v[0] = 32;
    return fr29_from_plain(mul(y_mont, to_mont(c32)));
}
static Fr29 fr29_mont_of(const Fr8& y_mont) { return fr29_mont_of(as_fr(y_mont)); }
// the INTEGER 32 s mod r for a value s given in the saturated Montgomery form: mul(Y, .) = y s for a stored Y = y 2^256 (k_fk20_scalars)
static Fr29 fr29_int32x_of(const Fr8& s_mont) {
    Fr c32 = zero<FrParams>();
    c32.v[0] = 32;
    return fr29_from_plain(from_mont(mul(as_fr(s_mont), to_mont(c32))));
}
static NttConsts ntt_consts(const Fr8& n_inv_mont) {
    NttConsts K;
    K.ninv_to_sat = fr29_mont_of(to_mont(as_fr(n_inv_mont)));     // (n^-1 2^256) 2^261: the Montgomery form of the INTEGER n^-1 2^256 mod r, times 32
    K.ninv_plain = fr29_mont_of(n_inv_mont);                      // n^-1 2^261
    K.one = fr29_mont_of(one<FrParams>());                        // 2^261 (one<>() is the Montgomery form of 1)
    return K;
}
void ntt_twiddles29(const void* w8192_mont_host /*Fr[8192]*/, void* out_host /*8192 x 9 words*/) {
    const Fr* w = (const Fr*)w8192_mont_host;
    Fr29* o = (Fr29*)out_host;
    for (int k = 0; k < N_EXT; k++) o[k] = fr29_mont_of(*(const Fr8*)&w[k]);
}
void blob_to_coeffs(int n, const uint8_t* blobs, void* coeffs, void* canon, int* status, const void* w29, const Fr8& n_inv, hipStream_t st) {
    k_blob_to_coeffs<<<n, 1024, LDS_NTT29, st>>>(blobs, (Fr*)coeffs, (Fr*)canon, status, (const Fr29*)w29, ntt_consts(n_inv));
}
void blob_eval_at(int n, const uint8_t* blobs, const void* z_mont, uint8_t* y_be32, void* y_mont, int* bad, const void* w29, const Fr8& n_inv,
                  hipStream_t st) {
    if (n > 0) k_blob_eval_at<<<n, 1024, LDS_NTT29, st>>>(blobs, (const Fr*)z_mont, y_be32, (Fr*)y_mont, bad, (const Fr29*)w29, ntt_consts(n_inv));
}
void blob_to_extension(int n, uint8_t* cells, int* status, const void* w29, const Fr8& n_inv, hipStream_t st) {
    if (n > 0) k_blob_to_extension<<<n, 1024, LDS_NTT29, st>>>(cells, status, (const Fr29*)w29, ntt_consts(n_inv));
}
void blob_to_columns(int n, const uint8_t* blobs, uint8_t* cells, const Columns& cols, bool blob_half, int* status, const void* w29, const Fr8& n_inv,
                     hipStream_t st) {
    if (n <= 0) return;
    const CellsByColumn dst{cells, cols.n_total, cols.b0};
    if (blob_half) k_blob_to_columns<true><<<n, 1024, LDS_NTT29, st>>>(blobs, dst, status, (const Fr29*)w29, ntt_consts(n_inv));
    else k_blob_to_columns<false><<<n, 1024, LDS_NTT29, st>>>(blobs, dst, status, (const Fr29*)w29, ntt_consts(n_inv));
}
void cells_to_columns(int n, const uint8_t* src, uint8_t* cells, const Columns& cols, hipStream_t st) {
    if (n <= 0) return;
    const int vec16 = ((uintptr_t)cells & 15) == 0;  // (every cell of the matrix starts a multiple of 2048 from there)
    k_cells_to_columns<<<dim3(n, N_CELLS), 128, 0, st>>>(src, CellsByColumn{cells, cols.n_total, cols.b0}, vec16);
}
void proofs_to_columns(int n, const uint8_t* proofs, uint8_t* out, const Columns& cols, hipStream_t st) {
    if (n <= 0) return;
    const size_t bytes = (size_t)n * N_CELLS * 48;
    if ((((uintptr_t)proofs | (uintptr_t)out) & 3) == 0)
        k_proofs_to_columns<uint32_t><<<(unsigned)((bytes / 4 + 255) / 256), 256, 0, st>>>((const uint32_t*)proofs, (uint32_t*)out, cols.n_total, cols.b0, bytes / 4);
    else
        k_proofs_to_columns<uint8_t><<<(unsigned)((bytes + 255) / 256), 256, 0, st>>>(proofs, out, cols.n_total, cols.b0, bytes);
}
void coeffs_to_cells(int n, const void* coeffs, uint8_t* cells, const void* w29, hipStream_t st, const Columns* cols) {
    if (cols) k_coeffs_to_cells<<<dim3(n, 2), 1024, LDS_NTT29, st>>>((const Fr*)coeffs, CellsByColumn{cells, cols->n_total, cols->b0}, (const Fr29*)w29);
    else k_coeffs_to_cells<<<dim3(n, 2), 1024, LDS_NTT29, st>>>((const Fr*)coeffs, CellsByBlob{cells}, (const Fr29*)w29);
}
void fk20_scalars(int n, const void* coeffs, void* scalars, const void* w29, const Fr8& inv128, int segs, const Fr8* seg_shifts,
                  hipStream_t st) {
    SegShifts sh;
    for (int i = 0; i < 3; i++) sh.p[i] = fr29_mont_of(seg_shifts[i]);
    k_fk20_scalars<<<n * 16, 256, 0, st>>>((const Fr*)coeffs, (Fr*)scalars, (const Fr29*)w29, fr29_int32x_of(inv128), n, segs, sh);
}
void fk20_tap_consts(const void* w29, const Fr8& scale, void* out, hipStream_t st) {
    k_fk20_tap_consts<<<2 * N_BLOB / 256, 256, 0, st>>>((const Fr29*)w29, fr29_from_plain(from_mont(as_fr(scale))), (Fr29*)out);
}
void coeffs_to_blobs(int n, const void* coeffs, uint8_t* blobs, const void* w29, hipStream_t st) {
    k_coeffs_to_cells<<<dim3(n, 1), 1024, LDS_NTT29, st>>>((const Fr*)coeffs, BlobsOnly{blobs}, (const Fr29*)w29);  // blockIdx.y = 0: half 0 alone
}
void coeffs_to_cells_scalars(int n, const void* coeffs, uint8_t* cells, void* scalars, const uint8_t* blobs, const int* status, const void* w29,
                             const void* tapk, int segs, const Fr8* seg_shifts, hipStream_t st, const Columns* cols) {
    // the 16-byte copy of an accepted blob wants both ends aligned and apart (a caller may hand in any byte address, and cells that
    // overlap the blobs were fine while every blob was read before the first cell was written): otherwise every block transforms
    // (column layout: `cells` is the whole call's array, n_total blobs wide, and every cell of it starts on a multiple of 2048 from there)
    const uintptr_t pb = (uintptr_t)blobs, pc = (uintptr_t)cells;
    const size_t cells_bytes = (cols ? cols->n_total : (size_t)n) * N_EXT * 32;
    const bool apart = pb + (size_t)n * BYTES_PER_BLOB <= pc || pc + cells_bytes <= pb;
    if (!status || ((pb | pc) & 15) || !apart) blobs = nullptr;
    SegShifts sh;
    for (int i = 0; i < 3; i++) sh.p[i] = fr29_mont_of(seg_shifts[i]);
    if (cols)
        k_coeffs_to_cells_scalars<<<dim3(n, 2), 1024, LDS_NTT29, st>>>((const Fr*)coeffs, CellsByColumn{cells, cols->n_total, cols->b0}, (Fr*)scalars, blobs,
                                                                       status, (const Fr29*)w29, (const Fr29*)tapk, n, segs, sh);
    else
        k_coeffs_to_cells_scalars<<<dim3(n, 2), 1024, LDS_NTT29, st>>>((const Fr*)coeffs, CellsByBlob{cells}, (Fr*)scalars, blobs, status, (const Fr29*)w29,
                                                                       (const Fr29*)tapk, n, segs, sh);
}
#ifdef KZG_TEST_HOOKS
void test_ntt4096(const uint8_t* in, uint8_t* out, const void* w29, const Fr8& n_inv, int inverse_dit, hipStream_t st) {
    k_test_ntt4096<<<1, 1024, LDS_NTT29, st>>>(in, out, (const Fr29*)w29, ntt_consts(n_inv), inverse_dit);
}
void test_scalars_be(const uint8_t* in, void* out, size_t n, hipStream_t st) {
    k_test_scalars_be<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(in, (Fr*)out, n);
}
void test_field_mul(const uint8_t* a, const uint8_t* b, uint8_t* out, int n, int is_fp, hipStream_t st) {
    if (is_fp) k_test_field_mul<Fp><<<(n + 63) / 64, 64, 0, st>>>(a, b, out, n);
    else k_test_field_mul<Fr><<<(n + 63) / 64, 64, 0, st>>>(a, b, out, n);
}
#endif
}  // namespace launch
}  // namespace kzg
