// Kernels of eth_kzg_amd_verify_kzg_proof_many: MANY independent verify_kzg_proof items in one pass (point_many.hip), a verdict each.
// Per item i the equation of Verifier::verify_kzg_proof (crates/cryptography/kzg_single_open/src/verifier.rs:33-57), in the shape
// eip4844.hip evaluates it,  e(pi_i, [tau]_2) e(C_i + z_i pi_i - y_i G, -[1]_2) = 1,  weighted by the pass's 127-bit rho_i
// (verify_host.hpp: PointProofTranscript): the item's pair is
//     ( rho_i pi_i ,  rho_i C_i + (rho_i z_i) pi_i - (rho_i y_i) G )
// Decoding and subgroup tests of [proofs | commitments] and the parsing of z and y are the existing kernels (k_g1misc.hip, k_4844.hip);
// the leaves are hashed by k_sha256_many; the folds and the probes of the search are k_vm_fold_ranges (k_verify_many.hip) over the
// pairs this file leaves in HBM.  This file adds:
//   k_pm_leaf_bodies  the 176 bytes "RCKZGPROOFLEAF_1" | C_i | z_i | y_i | pi_i of every leaf, gathered for k_sha256_many (device form)
//   k_pm_status       the item's status in the single call's order: 2 a point is no canonical subgroup point, else 1 z or y >= r, else 0
//   k_pm_blob_status  the same for an item that came as a blob: 1 the blob holds an element >= r, else 2 a point is bad, else 0
//   k_pm_mul          ONE LANE PER SCALAR MULTIPLICATION, four per item, with the per-lane GLV multiplication of vm_lane_mul.hpp:
//                     rho pi and rho C (127 bits: k1 only), (rho z mod r) pi and (rho y mod r) G (255 bits, balanced halves).  The G
//                     term is taken PER ITEM, so that the pair of every range is a plain sum of resident pairs.  The lanes of a wave
//                     hold products of one kind (the kinds lie one behind the other), so a wave's lanes run the same length
//   k_pm_pairs        per item: the second sum, with the exact addition (C + z pi is a doubling, the identity, or equals y G in the
//                     tests' degenerate items); an item whose status is not 0 leaves the identity pair and takes no part in any sum
#include "engine.hpp"
#include "kcommon.hpp"
#include "curve29.hpp"
#include "launch.hpp"
#include "glv.hpp"
#include "vm_lane_mul.hpp"

namespace kzg {

namespace {
constexpr uint32_t le32_of(const char* s) {
    return (uint32_t)(uint8_t)s[0] | ((uint32_t)(uint8_t)s[1] << 8) | ((uint32_t)(uint8_t)s[2] << 16) | ((uint32_t)(uint8_t)s[3] << 24);
}
constexpr int LEAF_WORDS = 44;  // 16 + 48 + 32 + 32 + 48 bytes
}  // namespace

// one thread per 32-bit word of a body; every source array is 4-byte aligned (they lie in the pass's arena)
__global__ __launch_bounds__(256) void k_pm_leaf_bodies(const uint32_t* __restrict__ commitments, const uint32_t* __restrict__ zs,
                                                        const uint32_t* __restrict__ ys, const uint32_t* __restrict__ proofs,
                                                        uint32_t* __restrict__ bodies, int n) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n * LEAF_WORDS) return;
    const size_t i = t / LEAF_WORDS;
    const int w = (int)(t - i * LEAF_WORDS);
    uint32_t v;
    if (w < 4) v = w == 0 ? le32_of("RCKZ") : w == 1 ? le32_of("GPRO") : w == 2 ? le32_of("OFLE") : le32_of("AF_1");
    else if (w < 16) v = commitments[i * 12 + (w - 4)];
    else if (w < 24) v = zs[i * 8 + (w - 16)];
    else if (w < 32) v = ys[i * 8 + (w - 24)];
    else v = proofs[i * 12 + (w - 32)];
    bodies[t] = v;
}

// point_status: [proofs n | commitments n] as the decoding left them (0 = a canonical point of the subgroup)
__global__ __launch_bounds__(256) void k_pm_status(const int* __restrict__ point_status, const int* __restrict__ z_bad, const int* __restrict__ y_bad,
                                                   int* __restrict__ status, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    status[i] = (point_status[n + i] || point_status[i]) ? ERR_G1 : (z_bad[i] || y_bad[i]) ? ERR_SCALAR : OK;
}

// The blob source: z and y are the verifier's own, so only the blob and the points can refuse an item, the blob first (verify_host.hpp:
// blob_item_status; crates/eip4844/src/verifier.rs:49-74).  One lane per item; a lane behind the last item repeats it and stores nothing.
__global__ __launch_bounds__(256) void k_pm_blob_status(const int* __restrict__ point_status, const int* __restrict__ blob_bad,
                                                        int* __restrict__ status, int n) {
    const int lane = blockIdx.x * 256 + threadIdx.x;
    const int i = lane < n ? lane : n - 1;
    const int s = blob_bad[i] ? ERR_SCALAR : (point_status[n + i] || point_status[i]) ? ERR_G1 : OK;
    if (lane < n) status[i] = s;
}

// products e < n: rho_e pi_e -> pairs[2 e];  then into terms: n <= e < 2n: rho C;  2n <= e < 3n: (rho z) pi;  3n <= e < 4n: (rho y) G.
// pts = [proofs n | commitments n] affine Montgomery-384 (decoded); z, y Montgomery; rho: four words per item, below 2^127.
// A lane behind the last product repeats its work and stores nothing.
__global__ __launch_bounds__(64, 2) void k_pm_mul(const G1Affine* __restrict__ pts, const G1Affine* __restrict__ gen, const Fr* __restrict__ z_mont,
                                                  const Fr* __restrict__ y_mont, const uint32_t* __restrict__ rho, const int* __restrict__ status,
                                                  JacQ* __restrict__ pairs, JacQ* __restrict__ terms, int n, Fq<1> beta) {
    const long lane = (long)blockIdx.x * 64 + threadIdx.x;
    const long e = lane < 4L * n ? lane : 4L * n - 1;
    const int kind = (int)(e / n), i = (int)(e - (long)kind * n);
    JacQ r = jacq_inf();
    if (status[i] == 0) {
        uint32_t split[8] = {rho[4 * (size_t)i], rho[4 * (size_t)i + 1], rho[4 * (size_t)i + 2], rho[4 * (size_t)i + 3] & 0x7fffffffu, 0, 0, 0, 0};
        if (kind >= 2) {
            Fr w = zero<FrParams>();  // the weight as a plain integer: times a Montgomery value, the product comes out plain
#pragma unroll
            for (int l = 0; l < 4; l++) w.v[l] = split[l];
            glv_split_balanced(mul(w, kind == 2 ? z_mont[i] : y_mont[i]), split);
        }
        const G1Affine P = kind == 3 ? *gen : pts[kind == 1 ? n + i : i];
        r = vm_mul_by_scalar(affq_from_affine(P), split, beta, VmLane());
    }
    if (lane >= 4L * n) return;
    if (kind == 0) pairs[2 * (size_t)i] = r;
    else terms[(size_t)(kind - 1) * n + i] = r;
}

// pairs[2 i + 1] = rho C + (rho z) pi - (rho y) G
__global__ __launch_bounds__(64) void k_pm_pairs(const JacQ* __restrict__ terms, JacQ* __restrict__ pairs, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    pairs[2 * (size_t)i + 1] = add(add(terms[i], terms[(size_t)n + i]), terms[2 * (size_t)n + i], /*negq=*/true);
}

namespace launch {
void preload_k_point_many() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_pm_mul));
}
void pm_leaf_bodies(const uint8_t* commitments, const uint8_t* zs, const uint8_t* ys, const uint8_t* proofs, uint8_t* bodies, int n, hipStream_t st) {
    if (n <= 0) return;
    const size_t words = (size_t)n * LEAF_WORDS;
    k_pm_leaf_bodies<<<(unsigned)((words + 255) / 256), 256, 0, st>>>((const uint32_t*)commitments, (const uint32_t*)zs, (const uint32_t*)ys,
                                                                     (const uint32_t*)proofs, (uint32_t*)bodies, n);
}
void pm_status(const int* point_status, const int* z_bad, const int* y_bad, int* status, int n, hipStream_t st) {
    if (n > 0) k_pm_status<<<(n + 255) / 256, 256, 0, st>>>(point_status, z_bad, y_bad, status, n);
}
void pm_blob_status(const int* point_status, const int* blob_bad, int* status, int n, hipStream_t st) {
    if (n > 0) k_pm_blob_status<<<(n + 255) / 256, 256, 0, st>>>(point_status, blob_bad, status, n);
}
void pm_mul(const void* pts, const void* gen, const void* z_mont, const void* y_mont, const uint32_t* rho, const int* status, void* pairs, void* terms,
            int n, const Fp12w& beta, hipStream_t st) {
    if (n <= 0) return;
    k_pm_mul<<<(unsigned)((4L * n + 63) / 64), 64, 0, st>>>((const G1Affine*)pts, (const G1Affine*)gen, (const Fr*)z_mont, (const Fr*)y_mont, rho, status,
                                                          (JacQ*)pairs, (JacQ*)terms, n, vm_beta(beta));
}
void pm_pairs(const void* terms, void* pairs, int n, hipStream_t st) {
    if (n > 0) k_pm_pairs<<<(n + 63) / 64, 64, 0, st>>>((const JacQ*)terms, (JacQ*)pairs, n);
}
}  // namespace launch
}  // namespace kzg
