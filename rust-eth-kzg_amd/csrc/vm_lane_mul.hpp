// k P for a PER-LANE scalar, one lane per product: the multiplication of the many-verifications (k_verify_many.hip: the cell
// verifier's products and its fold; k_point_many.hip: the products of eth_kzg_amd_verify_kzg_proof_many).  Device code in the
// verifier's 14 x 29-bit field; include behind curve29.hpp.
#pragma once
#include "curve29.hpp"

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
__device__ __forceinline__ JacQ vm_step(const JacQ& t, const AffQ& p) { return add_mixed(t, p); }
__device__ __forceinline__ JacQ vm_step(const JacQ& t, const JacQ& p) { return add(t, p); }
__device__ __forceinline__ JacQ vm_lift(const AffQ& p) { return to_jacq(p); }
__device__ __forceinline__ JacQ vm_lift(const JacQ& p) { return p; }
template <class Base>  // AffQ (decoded input points) or JacQ (sums that are multiplied again: the folded pairing inputs)
__device__ JacQ vm_mul_by_scalar(const Base& P, const uint32_t split[8], const Fq<1>& beta) {
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
            T[j] = j == 1 ? dbl(T[0]) : vm_step(T[j - 1], P);
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
            for (int s = 0; s < 4; s++) acc = dbl(acc);
        }
        const int d1 = vm_booth4(m1, w), d2 = vm_booth4(m2, w);
        if (d1 != 0) acc = add_mixed(acc, A[(d1 < 0 ? -d1 : d1) - 1], (d1 < 0) != n1);
        if (d2 != 0) {
            AffQ2 op = A[(d2 < 0 ? -d2 : d2) - 1];
            op.x = bx[(d2 < 0 ? -d2 : d2) - 1];
            acc = add_mixed(acc, op, (d2 < 0) != n2);
        }
    }
    acc.z = relax<ZB>(mul(acc.z, zc));  // back from the isomorphic curve (an identity P gives zc = 0: the identity)
    return acc;
}

}  // namespace kzg
