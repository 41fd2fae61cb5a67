// Kernels of eth_kzg_amd_verify_cell_kzg_proof_batch_many: MANY independent verify_cell_kzg_proof_batch problems in one pass
// (the reference verifies concurrently from many threads on one context, bindings/node/src/lib.rs:92-299; here the
// problems ride side by side on the GPU).  Per problem b the equation of FK20Verifier::verify_multi_opening
// (crates/cryptography/kzg_multi_open/src/fk20/verifier.rs:129-260) needs two G1 sums,
//     A_b = sum_k r_b^k pi_k
//     B_b = sum_k r_b^k h_k^64 pi_k + sum_row w_row C_row - commit(sum_k r_b^k I_k)
// with its own Fiat-Shamir challenge r_b.  What does not depend on the challenge (point decoding, subgroup tests, cell
// decoding, per-cell interpolation) runs over the concatenation of all problems with the single-problem kernels of
// k_g1misc.hip / k_verify.hip; this file adds what is per problem:
//   k_vm_scalars      r_b^k, the two proof scalars, from a per-problem table of r_b^(2^i)
//   k_vm_weights      w_row = sum of r_b^k over the cells of that commitment (block per unique commitment, its problem's cells only)
//   k_vm_interp_sum   the 64 coefficients of sum_k r_b^k I_k per problem (block per problem), negated, canonical
//   k_vm_products     ONE LANE (or one quad, vm_lane_mul.hpp) PER (point, scalar) product: a verification of 128 cells is 257 independent
//                     scalar multiplications, a thousand of them fill the chip, so no bucket method and no sorting: GLV split, both
//                     halves in signed 4-bit fixed windows over ONE table of 1..8 P brought to a common Z (g1_mulc.hpp's
//                     isomorphic-curve trick): 128 doublings + 64 mixed additions, every lane in lockstep
//   k_vm_reduce       per problem: the two sums of its products (+ the fixed-base commitment of the interpolation polynomial,
//                     which comes from the commitment window table: the first 64 SRS points are its group 0)
#include "engine.hpp"
#include "kcommon.hpp"
#include "curve29.hpp"
#include "launch.hpp"
#include "glv.hpp"
#include "vm_lane_mul.hpp"

#include <stdexcept>

namespace kzg {

struct VmPow { Fr p[24]; };  // r^(2^i), Montgomery

// r_b^e out of the problem's table (compute_powers, verifier.rs:333-343)
__device__ __forceinline__ Fr vm_power(const VmPow* tab, int e) {
    Fr acc = one<FrParams>();
    for (int i = 0; i < 24; i++)
        if ((e >> i) & 1) acc = mul(acc, tab->p[i]);
    return acc;
}
__global__ void k_vm_scalars(const VmPow* __restrict__ tabs, const int* __restrict__ batch_of, const int* __restrict__ pos_in_batch,
                             const int* __restrict__ cell_idx, const Fr* __restrict__ w8192, Fr* __restrict__ rp_mont,
                             Fr* __restrict__ s1, Fr* __restrict__ s2, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const Fr acc = vm_power(tabs + batch_of[k], pos_in_batch[k]);
    rp_mont[k] = acc;
    s1[k] = from_mont(acc);
    // coset generator h_c = omega_8192^brp7(c) (cosets.rs:89-112); h_c^64 = omega_128^brp7(c) = w8192[64 * brp7(c)]
    const int bc = (int)(__brev((unsigned)cell_idx[k]) >> 25);
    s2[k] = from_mont(mul(acc, w8192[64 * bc]));
}

__device__ __forceinline__ Fr vm_block_sum(uint32_t (*part)[256], Fr acc, int t) {
#pragma unroll
    for (int l = 0; l < 8; l++) part[l][t] = acc.v[l];
    __syncthreads();
    for (int span = 128; span >= 1; span >>= 1) {
        if (t < span) {
            Fr a, b;
#pragma unroll
            for (int l = 0; l < 8; l++) { a.v[l] = part[l][t]; b.v[l] = part[l][t + span]; }
            a = add(a, b);
#pragma unroll
            for (int l = 0; l < 8; l++) part[l][t] = a.v[l];
        }
        __syncthreads();
    }
    Fr a;
#pragma unroll
    for (int l = 0; l < 8; l++) a.v[l] = part[l][0];
    return a;
}
// weights[r] = sum of r_b^k over the cells k of problem b whose commitment is u (verifier.rs:216-219), canonical, block per weight.
// Expanded source: r = u is a global row (problem's first row + local row) and b = row_batch[r];  column source (row_batch null):
// r = b n_u + u over the pass's one commitment list;  partial columns (pair_start set): r is a pair, b the column whose pairs
// [pair_start[b], pair_start[b + 1]) hold it (a search over the n_cols + 1 starts, the same for the whole block) and u = pair_u[r].
// [cell_start[b], cell_start[b + 1]) = that problem's cells
__device__ __forceinline__ int vm_pair_column(const int* __restrict__ pair_start, int n_cols, int r) {
    int lo = 0, hi = n_cols;  // the last b with pair_start[b] <= r: columns without pairs repeat a start and are passed over
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pair_start[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(256) void k_vm_weights(const Fr* __restrict__ rp_mont, const int* __restrict__ row,
                                                    const int* __restrict__ row_batch, const int* __restrict__ cell_start,
                                                    Fr* __restrict__ weights, int n_u, const int* __restrict__ pair_start,
                                                    const int* __restrict__ pair_u, int n_cols) {
    __shared__ uint32_t part[8][256];
    const int r = blockIdx.x, t = threadIdx.x;
    const int b = pair_start ? vm_pair_column(pair_start, n_cols, r) : row_batch ? row_batch[r] : r / n_u;
    const int u = pair_start ? pair_u[r] : row_batch ? r : r - b * n_u;
    const int lo = cell_start[b], hi = cell_start[b + 1];
    Fr acc = zero<FrParams>();
    for (int k = lo + t; k < hi; k += 256)
        if (row[k] == u) acc = add(acc, rp_mont[k]);
    acc = vm_block_sum(part, acc, t);
    if (t == 0) weights[r] = from_mont(acc);
}
// out[b][i] = -(sum_{k in b} r^k coef[k][i]), canonical: the scalars of the interpolation commitment (verifier.rs:348-384, :235)
__global__ __launch_bounds__(256) void k_vm_interp_sum(const Fr* __restrict__ coef, const Fr* __restrict__ rp_mont,
                                                       const int* __restrict__ cell_start, Fr* __restrict__ out_neg_canon) {
    __shared__ uint32_t s[4][8][64];
    const int b = blockIdx.x, q = threadIdx.x >> 6, i = threadIdx.x & 63;
    const int lo = cell_start[b], hi = cell_start[b + 1];
    Fr acc = zero<FrParams>();
    for (int k = lo + q; k < hi; k += 4) acc = add(acc, mul(coef[(size_t)k * 64 + i], rp_mont[k]));
#pragma unroll
    for (int l = 0; l < 8; l++) s[q][l][i] = acc.v[l];
    __syncthreads();
    if (q == 0) {
        for (int o = 1; o < 4; o++) {
            Fr x;
#pragma unroll
            for (int l = 0; l < 8; l++) x.v[l] = s[o][l][i];
            acc = add(acc, x);
        }
        out_neg_canon[(size_t)b * 64 + i] = from_mont(neg(acc));
    }
}

// The product k P itself, by a lane or by a quad: vm_lane_mul.hpp (vm_mul_by_scalar; k_point_many.hip takes it from there too).
// The products of a pass: at most four consecutive segments of the product index e, segment j = [seg[j - 1].end, seg[j].end):
// its i-th product is scalars[i] (canonical) times points[idx ? idx[i] : wrap ? i % wrap : i] (affine Montgomery-384, decoded); an
// empty segment repeats the end before it.  The sources differ in the map alone (launch::vm_products).
struct VmSeg { int end, wrap; const Fr* scalars; const G1Affine* points; const int* idx; };
struct VmProductMap { VmSeg seg[4]; };
// prod[e] for every e < seg[3].end, PER_BLOCK products per block; a lane behind the last product repeats it and stores nothing
// (whole waves).  SHORT-CHAIN passes (a handful of problems: concurrent single calls combined, verify_many.hip)
// are a chain of latencies, so the chain is cut: their ONE launch holds every scalar multiplication of the pass -- with, as 64 more
// products per problem, the terms isc[b][j] SRS_j of the interpolation commitments (one more 255-bit multiplication each instead of
// a window-table MSM launch of its own: 25 % more lanes, nothing on a chip that is empty anyway) -- AND, in the blocks from
// mul_blocks on, the subgroup tests of the decoded points pts[n_tests] (status 0 -> 0 / 2, others kept; their 126 dependent doublings
// run beside the multiplications' 128 instead of in front).  Other passes have no such blocks.
template <class Ops>
__global__ __launch_bounds__(64, 2) void k_vm_products(VmProductMap map, JacQ* __restrict__ prod, int mul_blocks, const G1Affine* __restrict__ pts,
                                                       int* __restrict__ status /*[n_tests]*/, int n_tests, Fq<1> beta) {
    const Ops ops;
    if ((int)blockIdx.x >= mul_blocks) {
        const int i = ((int)blockIdx.x - mul_blocks) * Ops::PER_BLOCK + ops.sub();
        if (i >= n_tests || status[i] != 0) return;
        const G1Affine a = pts[i];
        if (is_inf(a)) return;
        if (!ops.in_subgroup(affq_from_affine(a), beta)) status[i] = 2;
        return;
    }
    const int total = map.seg[3].end;
    int e = blockIdx.x * Ops::PER_BLOCK + ops.sub();
    const bool real = e < total;
    if (!real) e = total - 1;
    VmSeg s = map.seg[0];
    int i = e;
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (e >= map.seg[j - 1].end) { s = map.seg[j]; i = e - map.seg[j - 1].end; }
    uint32_t split[8];
    glv_split_balanced(s.scalars[i], split);
    const JacQ r = vm_mul_by_scalar(affq_from_affine(s.points[s.idx ? s.idx[i] : s.wrap ? i % s.wrap : i]), split, beta, ops);
    if (real) prod[e] = r;
}
// two trees of 128 partial sums side by side (job 0 in red[0..128), job 1 in red[128..256)), each folded by its half of the
// block with four lanes per addition (g1_coop.hpp: the idle lanes of a tree level share its additions); red[128 * job] = the sums
__device__ __forceinline__ void vm_two_trees(JacQ* red, int t, int first_span = 64) {
    const int job = t >> 7, l = t & 127, quad = l & 3, slot = l >> 2;  // 32 additions per round and half
    JacQ* mine = red + 128 * job;
    __syncthreads();
#pragma unroll 1
    for (int span = first_span; span >= 1; span >>= 1) {
#pragma unroll 1
        for (int base = 0; base < span; base += 32) {
            const int a = base + slot;
            if (a < span) {
                const JacQ r = coop_add(mine[a], mine[a + span], false, quad);
                if (quad == 0) mine[a] = r;
            }
        }
        __syncthreads();
    }
}
// per problem b: out[2b] = sum of prod[cells of b], out[2b + 1] = sum of prod[n + cells of b] + sum of prod[2n + rows of b]
// + (icommit ? icommit[b] : the problem's 64 interpolation terms prod[2n + m + 64 b ..], short-chain form); threads 0-127 take
// the first sum, 128-255 the second, 7-level trees in LDS
__global__ __launch_bounds__(256) void k_vm_reduce(const JacQ* __restrict__ prod, const JacQ* __restrict__ icommit,
                                                   const int* __restrict__ cell_start, const int* __restrict__ row_start,
                                                   JacQ* __restrict__ out, int n, int m) {
    __shared__ JacQ red[256];
    const int b = blockIdx.x, t = threadIdx.x, job = t >> 7, l = t & 127;
    const int lo = cell_start[b], hi = cell_start[b + 1], rlo = row_start[b], rhi = row_start[b + 1];
    JacQ acc = jacq_inf();
    const JacQ* src = prod + (job ? n : 0);
    for (int k = lo + l; k < hi; k += 128) acc = add(acc, src[k]);
    if (job) {
        for (int r = rlo + l; r < rhi; r += 128) acc = add(acc, prod[2 * (size_t)n + r]);
        const JacQ* last = icommit ? icommit + b : prod + 2 * (size_t)n + m + 64 * (size_t)b;
        if (l < (icommit ? 1 : 64)) acc = add(acc, last[l]);
    }
    red[t] = acc;
    vm_two_trees(red, t);
    if (l == 0) out[2 * (size_t)b + job] = red[128 * job];
}

// Folding the problems' pairing checks into ONE: with weights rho_b (128 bits, derived by the host from ALL the problems'
// challenges, 0 for a problem that is excluded) the 2 x B sums become  S_j = sum_b rho_b out[b][j],  and
// e(S_0, [tau^64]_2) e(S_1, -[1]_2) = 1 holds for every choice of weights iff every problem's own equation holds (up to 2^-128
// for weights the prover cannot predict: the same argument as the powers of r inside one batch, verifier.rs:148-160).
// k_vm_fold_mul: lane or quad = (problem, j): rho_b * out[b][j] (a 128-bit scalar: k1 only; the 2 B products of a pass of a few
// problems are a few waves on an idle chip, each a chain of 124 doublings and ~32 additions);  k_vm_fold_sum: one block, two trees.
template <class Ops>
__global__ __launch_bounds__(64, 2) void k_vm_fold_mul(const JacQ* __restrict__ sums, const uint32_t* __restrict__ rho /*[B][4]*/,
                                                       JacQ* __restrict__ prod, int n_batches, Fq<1> beta) {
    const Ops ops;
    const int e = blockIdx.x * Ops::PER_BLOCK + ops.sub();
    if (e >= 2 * n_batches) return;
    const int b = e >> 1;
    uint32_t split[8] = {rho[4 * b], rho[4 * b + 1], rho[4 * b + 2], rho[4 * b + 3] & 0x7fffffffu, 0, 0, 0, 0};
    prod[e] = vm_mul_by_scalar(sums[e], split, beta, ops);
}
__global__ __launch_bounds__(256) void k_vm_fold_sum(const JacQ* __restrict__ prod, JacQ* __restrict__ out2, int n_batches) {
    __shared__ JacQ red[256];
    const int t = threadIdx.x, job = t >> 7, l = t & 127;
    JacQ acc = jacq_inf();
    for (int b = l; b < n_batches; b += 128) acc = add(acc, prod[2 * (size_t)b + job]);
    red[t] = acc;
    vm_two_trees(red, t);
    if (l == 0) out2[job] = red[128 * job];
}

// sums of the weighted per-problem pairs over RANGES of problems: out[r][j] = sum of prod[b][j], ranges[r][0] <= b < ranges[r][1]
// (the probes of the search for the wrong proofs of a pass whose folded check failed; the products rho_b * sum_b are resident)
__global__ __launch_bounds__(256) void k_vm_fold_ranges(const JacQ* __restrict__ prod, const int* __restrict__ ranges, JacQ* __restrict__ out) {
    __shared__ JacQ red[256];
    const int t = threadIdx.x, job = t >> 7, l = t & 127;
    const int lo = ranges[2 * blockIdx.x], hi = ranges[2 * blockIdx.x + 1];
    JacQ acc = jacq_inf();
    for (int b = lo + l; b < hi; b += 128) acc = add(acc, prod[2 * (size_t)b + job]);
    const int width = hi - lo < 128 ? hi - lo : 128;  // lanes that hold anything
#pragma unroll 1
    for (int span = 64; span >= 1; span >>= 1) {
        if (span >= width) continue;  // (block-uniform) nothing to fold at this distance
        red[t] = acc;
        __syncthreads();
        if (l < span) acc = add(acc, red[t + span]);
        __syncthreads();
    }
    if (l == 0) out[2 * (size_t)blockIdx.x + job] = acc;
}

// ---- The columns of one block over ONE commitment list (eth_kzg_amd_verify_data_columns; verify_many.hip, the column source).
// Problem b is column b: all its cells carry the index c_b, so h_k^64 = h_(c_b)^64 is one value per column and
//     B_b = h_(c_b)^64 A_b + sum_row w_(b,row) C_row - commit(sum_k r_b^k I_k):
// one product per column behind the reduction of A_b where the expanded pass multiplies every proof a second time.  The n_u unique
// commitments are decoded once per pass; pts = [proofs n | commitments n_u], row[k] < n_u is pass-wide.
//   k_vc_scalars    r_b^k per cell (no second proof scalar), h_(c_b)^64 per column, canonical
//   k_vm_weights    w[b][u] = sum of r_b^k over the cells of column b whose commitment is u (block per (column, commitment))
//   k_vm_products   the map r^k pi_k | w[b][u] C_u | (short-chain form) the interpolation terms
//   k_vc_reduce     per column: A_b, and T_b = sum_u w[b][u] C_u - commit(...)
//   k_vc_hmul       quad per column: B_b = h^64 A_b + T_b, the only writer of the column's second result slot
// PARTIAL columns (eth_kzg_amd_verify_partial_data_columns) hold the blobs of their bitmap only: the (column, commitment) pairs that
// exist are a list (pair_start per column, pair_u per pair), one weight and one product per pair; nothing else differs.
__global__ void k_vc_scalars(const VmPow* __restrict__ tabs, const int* __restrict__ batch_of, const int* __restrict__ pos_in_batch,
                             const int* __restrict__ cell_idx, const int* __restrict__ cell_start, const Fr* __restrict__ w8192,
                             Fr* __restrict__ rp_mont, Fr* __restrict__ s1, Fr* __restrict__ h64, int n, int n_cols) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) {
        const Fr acc = vm_power(tabs + batch_of[k], pos_in_batch[k]);
        rp_mont[k] = acc;
        s1[k] = from_mont(acc);
    }
    if (k < n_cols) {  // h_c^64 = omega_128^brp7(c) = w8192[64 * brp7(c)] (k_vm_scalars); a column without cells (refused): 1
        const int lo = cell_start[k], hi = cell_start[k + 1];
        Fr h = one<FrParams>();
        if (lo < hi) h = w8192[64 * (int)(__brev((unsigned)cell_idx[lo]) >> 25)];
        h64[k] = from_mont(h);
    }
}
// per column b: out[2b] = A_b = sum of prod[cells of b];  tsum[b] = sum_u prod[n + b n_u + u] + (icommit ? icommit[b] : the 64
// interpolation terms prod[n + W + 64 b ..]), W = columns x n_u.  out[2b + 1] is left to k_vc_hmul.  Partial columns (pair_start
// set): the column's w C products are prod[n + pair_start[b] .. n + pair_start[b + 1]) and W is the pass's pairs.
__global__ __launch_bounds__(256) void k_vc_reduce(const JacQ* __restrict__ prod, const JacQ* __restrict__ icommit, const int* __restrict__ cell_start,
                                                   JacQ* __restrict__ out, JacQ* __restrict__ tsum, int n, int n_u, int W,
                                                   const int* __restrict__ pair_start) {
    __shared__ JacQ red[256];
    const int b = blockIdx.x, t = threadIdx.x, job = t >> 7, l = t & 127;
    JacQ acc = jacq_inf();
    if (!job) {
        const int lo = cell_start[b], hi = cell_start[b + 1];
        for (int k = lo + l; k < hi; k += 128) acc = add(acc, prod[k]);
    } else {
        const JacQ* wc = prod + n + (pair_start ? (size_t)pair_start[b] : (size_t)b * n_u);
        const int n_w = pair_start ? pair_start[b + 1] - pair_start[b] : n_u;
        for (int u = l; u < n_w; u += 128) acc = add(acc, wc[u]);
        if (icommit) { if (l == 0) acc = add(acc, icommit[b]); }
        else if (l < 64) acc = add(acc, prod[(size_t)n + W + 64 * (size_t)b + l]);
    }
    red[t] = acc;
    vm_two_trees(red, t);
    if (l == 0) {
        if (job) tsum[b] = red[128];
        else out[2 * (size_t)b] = red[0];
    }
}
// out[2b + 1] = h64[b] * out[2b] + tsum[b]: a full 255-bit product per column, four lanes each (the columns of a pass are a few
// waves); the identity goes through the product as any point does (Z = 0 stays 0)
__global__ __launch_bounds__(64, 2) void k_vc_hmul(JacQ* __restrict__ out, const JacQ* __restrict__ tsum, const Fr* __restrict__ h64, int n_cols,
                                                   Fq<1> beta) {
    const VmQuad ops;
    int b = blockIdx.x * VmQuad::PER_BLOCK + ops.sub();
    const bool real = b < n_cols;
    if (!real) b = n_cols - 1;
    uint32_t split[8];
    glv_split_balanced(h64[b], split);
    JacQ r = vm_mul_by_scalar(out[2 * (size_t)b], split, beta, ops);
    r = coop_add(r, tsum[b], false, ops.quad);
    if (real && ops.quad == 0) out[2 * (size_t)b + 1] = r;
}

namespace launch {
// the code object of this translation unit is loaded now (HIP loads a code object on the first launch of one of its kernels, and
// that load is an allocation: it would wait behind a table piece the builder thread is allocating)
void preload_k_verify_many() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_vm_scalars));
}
// The two sources of a pass share every launcher; the column source (problem b = column b over ONE commitment list of m entries, its
// Bc m weights at most the n cells' worth: verify_many.hip takes refused columns out of the call) is told by the null pointer noted
// at each.  A product count that does not fit the 32-bit indices throws before any launch.
static int vm_count(long long products, int n_batches) {
    if (products < 0 || n_batches < 0 || products + 65LL * n_batches > 0x7fffffffLL) throw std::runtime_error("many-verification pass: too many products");
    return (int)products;
}
void vm_scalars(const void* pow_tables /*[B][24] Fr, device*/, const int* batch_of, const int* pos_in_batch, const int* cell_idx, const int* cell_start,
                const void* w8192, void* rp_mont, void* s1, void* s2, void* h64, int n, int n_batches, hipStream_t st) {
    const int lanes = h64 && n_batches > n ? n_batches : n;
    if (lanes <= 0) return;
    if (h64)
        k_vc_scalars<<<(lanes + 255) / 256, 256, 0, st>>>((const VmPow*)pow_tables, batch_of, pos_in_batch, cell_idx, cell_start, (const Fr*)w8192,
                                                           (Fr*)rp_mont, (Fr*)s1, (Fr*)h64, n, n_batches);
    else
        k_vm_scalars<<<(lanes + 255) / 256, 256, 0, st>>>((const VmPow*)pow_tables, batch_of, pos_in_batch, cell_idx, (const Fr*)w8192, (Fr*)rp_mont,
                                                           (Fr*)s1, (Fr*)s2, n);
}
void vm_weights(const void* rp_mont, const int* row, const int* row_batch, const int* cell_start, void* weights, int m, int n_batches, hipStream_t st,
                const VmPairs& pairs) {
    const int blocks = pairs.start ? vm_count(pairs.count, n_batches) : row_batch ? m : vm_count((long long)n_batches * m, n_batches);
    if (blocks > 0)
        k_vm_weights<<<blocks, 256, 0, st>>>((const Fr*)rp_mont, row, row_batch, cell_start, (Fr*)weights, m, pairs.start, pairs.u, n_batches);
}
void vm_interp_sum(const void* coef, const void* rp_mont, const int* cell_start, void* out_neg_canon, int n_batches, hipStream_t st) {
    if (n_batches > 0) k_vm_interp_sum<<<n_batches, 256, 0, st>>>((const Fr*)coef, (const Fr*)rp_mont, cell_start, (Fr*)out_neg_canon);
}
int vm_products(const void* pts, const void* s1, const void* s2, const void* wts, const void* isc, const void* srs, void* prod, int n, int m,
                int n_batches, bool small, int* status, const Fp12w& beta, hipStream_t st, const VmPairs& pairs) {
    const G1Affine* p = (const G1Affine*)pts;
    const long long W = pairs.start ? pairs.count : s2 ? m : (long long)n_batches * m, both = s2 ? 2LL * n : n;
    const int decoded = vm_count(n < 0 || m < 0 ? -1 : both + W, n_batches), proofs = (int)both;
    const int total = decoded + (small ? 64 * n_batches : 0), tests = small ? n + m : 0;
    if (total <= 0) return 0;
    const VmProductMap map = {{{n, 0, (const Fr*)s1, p, nullptr}, {proofs, 0, (const Fr*)s2, p, nullptr},
                               {decoded, s2 ? 0 : m, (const Fr*)wts, p + n, pairs.u}, {total, 64, (const Fr*)isc, (const G1Affine*)srs, nullptr}}};
    // quads up to 1,024 waves of 16 (products and tests): every wave still has a SIMD to itself
    const bool quads = small && total + tests <= 2 * coop_points_max();
    const int per = quads ? VmQuad::PER_BLOCK : VmLane::PER_BLOCK, mb = (total + per - 1) / per;
    const auto kernel = quads ? k_vm_products<VmQuad> : k_vm_products<VmLane>;
    kernel<<<mb + (tests + per - 1) / per, 64, 0, st>>>(map, (JacQ*)prod, mb, p, status, tests, vm_beta(beta));
    return decoded;
}
int vm_sums(const void* prod, const void* icommit, const int* cell_start, const int* row_start, const void* h64, void* out, int n, int m, int n_batches,
            const Fp12w& beta, hipStream_t st, const VmPairs& pairs) {
    if (n_batches <= 0) return 0;
    if (row_start) {
        k_vm_reduce<<<n_batches, 256, 0, st>>>((const JacQ*)prod, (const JacQ*)icommit, cell_start, row_start, (JacQ*)out, n, m);
        return 0;
    }
    const int W = pairs.start ? vm_count(pairs.count, n_batches) : vm_count((long long)n_batches * m, n_batches);
    JacQ* tsum = (JacQ*)prod + (size_t)n + W + (icommit ? 0 : 64 * (size_t)n_batches);
    k_vc_reduce<<<n_batches, 256, 0, st>>>((const JacQ*)prod, (const JacQ*)icommit, cell_start, (JacQ*)out, tsum, n, m, W, pairs.start);
    k_vc_hmul<<<(n_batches + 15) / 16, 64, 0, st>>>((JacQ*)out, tsum, (const Fr*)h64, n_batches, vm_beta(beta));
    return n_batches;
}
void vm_fold(const void* sums, const uint32_t* rho, void* prod, void* out2, int n_batches, const Fp12w& beta, hipStream_t st) {
    if (n_batches <= 0) return;
    if (2 * n_batches <= 2 * coop_points_max())
        k_vm_fold_mul<VmQuad><<<(2 * n_batches + 15) / 16, 64, 0, st>>>((const JacQ*)sums, rho, (JacQ*)prod, n_batches, vm_beta(beta));
    else k_vm_fold_mul<VmLane><<<(2 * n_batches + 63) / 64, 64, 0, st>>>((const JacQ*)sums, rho, (JacQ*)prod, n_batches, vm_beta(beta));
    k_vm_fold_sum<<<1, 256, 0, st>>>((const JacQ*)prod, (JacQ*)out2, n_batches);
}
void vm_fold_ranges(const void* prod, const int* ranges, void* out, int n_ranges, hipStream_t st) {
    if (n_ranges > 0) k_vm_fold_ranges<<<n_ranges, 256, 0, st>>>((const JacQ*)prod, ranges, (JacQ*)out);
}
}  // namespace launch
}  // namespace kzg
