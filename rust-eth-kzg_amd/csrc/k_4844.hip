// EIP-4844 single-point openings: quotient of the blob polynomial by (X - z) and its value at z.
// Reference: divide_by_linear (crates/cryptography/kzg_single_open/src/prover.rs:48-65, a sequential Ruffini
// recurrence) and PolyCoeff::eval (crates/cryptography/polynomial/src/poly_coeff.rs:59-65).
#include "engine.hpp"
#include "kcommon.hpp"
#include "launch.hpp"

namespace kzg {

// With H_k = sum_{j >= k} c_j z^(j-k) (so H_k = c_k + z H_{k+1}):  y = H_0 and quotient q_k = H_{k+1}.
// The recurrence is cut into 64 chunks of 64 coefficients: every lane runs the recurrence inside its chunk,
// lane 0 stitches the 64 chunk heads together with z^64, and every lane adds its carry-in times z^(distance).
// grid = n_blobs, block = 64.  quotient: [b][4096] canonical Fr (entry 4095 = 0) = the scalars of the MSM against
// the monomial SRS; y_out: [b] canonical.
__global__ __launch_bounds__(64) void k_quotient_by_linear(const Fr* __restrict__ coeffs, const Fr* __restrict__ z_mont,
                                                           Fr* __restrict__ quotient, Fr* __restrict__ y_out) {
    __shared__ Fr head[65];
    const int b = blockIdx.x, L = threadIdx.x;
    const Fr* c = coeffs + (size_t)b * N_BLOB;
    Fr* q = quotient + (size_t)b * N_BLOB;
    const Fr z = z_mont[b];
    // local recurrence, parked (Montgomery) in the output slots: slot k holds the chunk-local H_k
    Fr h = zero<FrParams>();
    for (int k = 64 * L + 63; k >= 64 * L; k--) {
        h = add(c[k], mul(z, h));
        q[k] = h;
    }
    head[L] = h;
    if (L == 0) head[64] = zero<FrParams>();
    __syncthreads();
    if (L == 0) {
        Fr z64 = z;
        for (int i = 0; i < 6; i++) z64 = sqr(z64);
        for (int l = 62; l >= 0; l--) head[l] = add(head[l], mul(z64, head[l + 1]));  // true H at every chunk boundary
    }
    __syncthreads();
    const Fr carry = head[L + 1];  // H_{64(L+1)}
    Fr pw = z;
    // second sweep, top-down: true H_k = local + z^(64L+64-k) * carry, kept in place (Montgomery) for now
    for (int k = 64 * L + 63; k >= 64 * L; k--) {
        q[k] = add(q[k], mul(pw, carry));
        pw = mul(pw, z);
    }
    __syncthreads();
    // shift by one and leave Montgomery form: q_k = H_{k+1}
    // (each lane only needs one value from its upper neighbour: read it before anyone overwrites)
    const Fr next_head = L < 63 ? q[64 * L + 64] : zero<FrParams>();
    const Fr y = q[0];
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < 64; i++) {
        const int k = 64 * L + i;
        const Fr v = i < 63 ? q[k + 1] : next_head;  // q[k+1] of this lane's own chunk is still H_{k+1}: ascending order
        q[k] = from_mont(v);
    }
    if (L == 0) y_out[b] = from_mont(y);
}

// The evaluation points of a batch, made on the device so that k_quotient_by_linear reads them from HBM without a host round trip.
// in: n x 32 bytes, big-endian (4-byte aligned).  One lane per value; the lanes behind the last one repeat its work and store nothing.
//   reduce != 0  the device twin of reduce_be32_4844 (eip4844.hip; reduce_bytes_to_scalar_bias): the 256-bit value mod r -- a
//                SHA-256 digest becomes the Fiat-Shamir challenge.  bad is not touched.
//   reduce == 0  deserialize_bytes_to_scalar (serialization/src/lib.rs:50-63): a value >= r is not canonical: bad[i] = 1 and the
//                point is 0 (the blob is still opened, its outputs are unspecified), else bad[i] = 0.
__global__ __launch_bounds__(64) void k_fr_from_be32(const uint8_t* __restrict__ in, Fr* __restrict__ out_mont, int* __restrict__ bad, int n,
                                                     int reduce) {
    const int lane_item = blockIdx.x * 64 + threadIdx.x;
    const int i = lane_item < n ? lane_item : n - 1;
    Fr x = load_fr_be(in + (size_t)i * 32);
    int flag = 0;
    if (reduce) {
        while (geq_mod<FrParams>(x.v)) {  // 2^256 < 6 r: at most five rounds
            Fr t;
            sub_limbs<8>(t.v, x.v, FrParams::MOD);
            x = t;
        }
    } else if (geq_mod<FrParams>(x.v)) {
        flag = 1;
        x = zero<FrParams>();
    }
    if (lane_item >= n) return;
    out_mont[i] = to_mont(x);
    if (!reduce) bad[i] = flag;
}
// canonical Fr -> 32 big-endian bytes (the y of compute_kzg_proof as the ABI hands it out)
__global__ __launch_bounds__(64) void k_fr_to_be32(const Fr* __restrict__ canon, uint8_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) store_fr_be(out + (size_t)i * 32, canon[i]);
}
// Montgomery Fr -> 32 big-endian canonical bytes (a challenge reduced on the device, as the point many-verification's leaves hash it)
__global__ __launch_bounds__(64) void k_fr_mont_to_be32(const Fr* __restrict__ mont, uint8_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) store_fr_be(out + (size_t)i * 32, from_mont(mont[i]));
}
// per-blob status of a batched opening in the single call's order (eip4844/src/prover.rs:37-92): 1 the blob holds a non-canonical
// element, else 1 the evaluation point is not canonical (z_bad; null: a hashed challenge), else 2 the commitment is not a valid
// subgroup point (g1_bad; null: none given), else 0
__global__ __launch_bounds__(64) void k_4844_status(const int* __restrict__ blob_bad, const int* __restrict__ z_bad,
                                                    const int* __restrict__ g1_bad, int* __restrict__ out, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    int s = 0;
    if (blob_bad[i]) s = ERR_SCALAR;
    else if (z_bad && z_bad[i]) s = ERR_SCALAR;
    else if (g1_bad && g1_bad[i]) s = ERR_G1;
    out[i] = s;
}

namespace launch {
void fr_from_be32(int n, const uint8_t* in, void* out_mont, int* bad, bool reduce, hipStream_t st) {
    if (n > 0) k_fr_from_be32<<<(n + 63) / 64, 64, 0, st>>>(in, (Fr*)out_mont, bad, n, reduce ? 1 : 0);
}
void fr_to_be32(int n, const void* canon, uint8_t* out, hipStream_t st) {
    if (n > 0) k_fr_to_be32<<<(n + 63) / 64, 64, 0, st>>>((const Fr*)canon, out, n);
}
void fr_mont_to_be32(int n, const void* mont, uint8_t* out, hipStream_t st) {
    if (n > 0) k_fr_mont_to_be32<<<(n + 63) / 64, 64, 0, st>>>((const Fr*)mont, out, n);
}
void status_4844(int n, const int* blob_bad, const int* z_bad, const int* g1_bad, int* out, hipStream_t st) {
    if (n > 0) k_4844_status<<<(n + 63) / 64, 64, 0, st>>>(blob_bad, z_bad, g1_bad, out, n);
}
// the code object of this translation unit is loaded now (HIP loads a code object on the first launch of one of its kernels, and
// that load is an allocation: it would wait behind a table piece the builder thread is allocating)
void preload_k_4844() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_quotient_by_linear));
}
void quotient_by_linear(int n, const void* coeffs, const void* z_mont, void* quotient, void* y_out, hipStream_t st) {
    k_quotient_by_linear<<<n, 64, 0, st>>>((const Fr*)coeffs, (const Fr*)z_mont, (Fr*)quotient, (Fr*)y_out);
}
}  // namespace launch
}  // namespace kzg
