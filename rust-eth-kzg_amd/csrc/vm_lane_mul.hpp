// k P for a PER-LANE scalar, by one lane or by the four lanes of a quad: the multiplication of the many-verifications
// (k_verify_many.hip: the cell verifier's products and its fold; k_point_many.hip: the products of eth_kzg_amd_verify_kzg_proof_many).
// Device code in the verifier's 14 x 29-bit field; include behind curve29.hpp.
#pragma once
#include "engine.hpp"
#include "curve29.hpp"
#include "g1_subgroup.hpp"
#include "g1_coop.hpp"

namespace kzg {

// signed Booth digit of 4-bit window w (< 32) of a 127-bit magnitude held in four words (bit 127 = sign, masked by the caller)
__device__ __forceinline__ int vm_booth4(const uint32_t m[4], int w) {
    uint32_t x;
    if (w == 0) x = (m[0] << 1) & 0x1fu;
    else {
        const int lo = 4 * w - 1, word = lo >> 5, sh = lo & 31;
        uint64_t two = m[word];
        if (word + 1 < 4) two |= (uint64_t)m[word + 1] << 32;
        x = (uint32_t)(two >> sh) & 0x1fu;
    }
    const int t = (int)((x + 1) >> 1);
    return (x >> 4) ? t - 16 : t;
}
// k P for a PER-LANE scalar k = s1 m1 + s2 m2 lambda (balanced GLV halves, glv.hpp): the table (j + 1) P, j < 8, is built with
// mixed additions (P is affine) and brought to one common Z without an inversion -- (X_j l_j^2, Y_j l_j^3), l_j = Z / z_j,
// are affine coordinates on the isomorphic curve y^2 = x^3 + 4 Z^6, whose group law (a = 0) and endomorphism are the same
// (g1_mulc.hpp) -- so the 64 additions of the main loop are mixed additions too.  All lanes run the same 32 windows:
// 4 doublings, one addition for k1's digit, one for k2's (phi of a table entry only swaps in beta x); a zero digit masks its lane.
// Who multiplies: ONE LANE per product (VmLane), or the FOUR LANES OF A QUAD (VmQuad, g1_coop.hpp) for the small passes whose waves
// have a SIMD each: the doublings and the mixed additions of the main loop and of the table are shared (3.5 and 5.5 multiplication
// times instead of 6.5 and 10.5), the table's common-Z step is repeated on every lane.  All four lanes hold the same P and the same
// scalar, so the digit tests are uniform in the quad, and every lane ends with the whole result.  sub() = the product of the block
// that this lane works on, PER_BLOCK of them in a block of 64 lanes.  The multiplication is a call: it takes the policy by value,
// which is nothing for a lane and the lane's place in its quad for a quad.
struct VmLane {
    static constexpr int PER_BLOCK = 64;
    __device__ __forceinline__ int sub() const { return threadIdx.x; }
    __device__ __forceinline__ JacQ dbl(const JacQ& p) const { return kzg::dbl(p); }
    template <class Aff> __device__ __forceinline__ JacQ add_mixed(const JacQ& p, const Aff& q, bool negq) const { return kzg::add_mixed(p, q, negq); }
    __device__ __forceinline__ JacQ step(const JacQ& t, const AffQ& p) const { return kzg::add_mixed(t, p); }
    __device__ __forceinline__ JacQ step(const JacQ& t, const JacQ& p) const { return kzg::add(t, p); }
    __device__ __forceinline__ bool in_subgroup(const AffQ& p, const Fq<1>& beta) const { return g1_in_subgroup_q(p, beta); }
};
struct VmQuad {
    static constexpr int PER_BLOCK = 16;
    const int quad;
    __device__ __forceinline__ VmQuad() : quad(threadIdx.x & 3) {}
    __device__ __forceinline__ int sub() const { return threadIdx.x >> 2; }
    __device__ __forceinline__ JacQ dbl(const JacQ& p) const { return coop_dbl(p, quad); }
    template <class Aff> __device__ __forceinline__ JacQ add_mixed(const JacQ& p, const Aff& q, bool negq) const { return coop_add_mixed(p, q, negq, quad); }
    __device__ __forceinline__ JacQ step(const JacQ& t, const AffQ& p) const { return coop_add_mixed(t, p, false, quad); }
    __device__ __forceinline__ JacQ step(const JacQ& t, const JacQ& p) const { return coop_add(t, p, false, quad); }
    __device__ __forceinline__ bool in_subgroup(const AffQ& p, const Fq<1>& beta) const { return g1_in_subgroup_coop(p, beta, quad); }
};
__device__ __forceinline__ JacQ vm_lift(const AffQ& p) { return to_jacq(p); }
__device__ __forceinline__ JacQ vm_lift(const JacQ& p) { return p; }
template <class Ops, class Base>  // Base: AffQ (decoded input points) or JacQ (sums that are multiplied again: the folded pairing inputs)
__device__ JacQ vm_mul_by_scalar(const Base& P, const uint32_t split[8], const Fq<1>& beta, const Ops ops) {
    constexpr int NT = 8;
    AffQ2 A[NT];
    Fq<2> bx[NT];
    Fq<ZB> zc;
    {
        JacQ T[NT];
        Fq<ZB> pre[NT];  // pre[j] = z_0 ... z_j
        T[0] = vm_lift(P);
        pre[0] = T[0].z;
#pragma unroll 1
        for (int j = 1; j < NT; j++) {
            T[j] = j == 1 ? ops.dbl(T[0]) : ops.step(T[j - 1], P);
            pre[j] = relax<ZB>(mul(pre[j - 1], T[j].z));
        }
        zc = pre[NT - 1];
        Fq<ZB> suf = relax<ZB>(fq_one());  // z_(j+1) ... z_(NT-1)
#pragma unroll 1
        for (int j = NT - 1; j >= 0; j--) {
            const Fq<ZB> lam = j > 0 ? relax<ZB>(mul(pre[j > 0 ? j - 1 : 0], suf)) : suf;  // product of all the other z
            const Fq<2> l2 = sqr(lam);
            A[j].x = mul(T[j].x, l2);
            A[j].y = mul(T[j].y, mul(l2, lam));
            bx[j] = mul(A[j].x, beta);
            suf = relax<ZB>(mul(suf, T[j].z));
        }
    }
    uint32_t m1[4] = {split[0], split[1], split[2], split[3] & 0x7fffffffu};
    uint32_t m2[4] = {split[4], split[5], split[6], split[7] & 0x7fffffffu};
    const bool n1 = (split[3] >> 31) != 0, n2 = (split[7] >> 31) != 0;
    JacQ acc = jacq_inf();
#pragma unroll 1
    for (int w = 31; w >= 0; w--) {
        if (w != 31) {
#pragma unroll 1
            for (int s = 0; s < 4; s++) acc = ops.dbl(acc);
        }
        const int d1 = vm_booth4(m1, w), d2 = vm_booth4(m2, w);
        if (d1 != 0) acc = ops.add_mixed(acc, A[(d1 < 0 ? -d1 : d1) - 1], (d1 < 0) != n1);
        if (d2 != 0) {
            AffQ2 op = A[(d2 < 0 ? -d2 : d2) - 1];
            op.x = bx[(d2 < 0 ? -d2 : d2) - 1];
            acc = ops.add_mixed(acc, op, (d2 < 0) != n2);
        }
    }
    acc.z = relax<ZB>(mul(acc.z, zc));  // back from the isomorphic curve (an identity P gives zc = 0: the identity)
    return acc;
}
// host side: the engine's beta (12 words, Montgomery-384) as the kernels take it
inline Fq<1> vm_beta(const Fp12w& beta) {
    Fp b384;
    for (int i = 0; i < 12; i++) b384.v[i] = beta.v[i];
    return fq_from_fp(b384);
}

}  // namespace kzg
