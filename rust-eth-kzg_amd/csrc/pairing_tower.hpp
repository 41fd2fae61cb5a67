// The ONE statement of the pairing's tower arithmetic, for the host (host_pairing.cpp) and for the device (k_pairing.hip), as
// verify_host.hpp is for the transcripts.  Tower Fp2 = Fp[u]/(u^2+1), Fp6 = Fp2[v]/(v^3-(1+u)), Fp12 = Fp6[w]/(w^2-v);
// M-type twist E'(Fp2): y^2 = x^3 + 4(1+u), untwist (x, y) -> (x / w^2, y / w^3).
// Here: Fp2 / Fp6 / Fp12 arithmetic, the sparse product with a line's value, the Miller loop over PREPARED lines, the final
// exponentiation's verdict, and check_lane -- what one lane of k_pairing_check computes.  G2 decompression, prepare() and the G2
// subgroup code stay in host_pairing.cpp: they run once per setup.
//
// On the device the Fp2 product and square, the Fp6 and Fp12 products and the Fp inversion are real functions (TW_NI): a check is
// ~16 k Fp multiplications, and inlining them all makes a code object nobody can load.  On the host the same bodies inline as they
// always did.
#pragma once
#include <cstdint>
#include "curve29.hpp"

namespace kzg {
namespace pairing {

struct Fp2 { Fp c0, c1; };                 // c0 + c1 u, u^2 = -1
struct Fp6 { Fp2 c0, c1, c2; };            // over Fp2, v^3 = 1 + u
struct Fp12 { Fp6 c0, c1; };               // over Fp6, w^2 = v
struct Line { Fp2 a, b; };                 // l(P) * w^3 = a + (b * xP) v + yP (v w)
// Frobenius: v^p = xi^((p-1)/3) v, w^p = xi^((p-1)/6) w
struct FrobConsts { Fp2 g1, g2, g4; };     // xi^((p-1)/6), its square, its fourth power
static_assert(sizeof(Line) == 192 && sizeof(Fp12) == 576 && sizeof(FrobConsts) == 288, "device layouts");

// |x| = 0xd201000000010000 (the BLS parameter is negative; see miller_loop_lines)
constexpr uint64_t X_ABS = 0xd201000000010000ULL;
constexpr int MILLER_LINES = 68;  // 63 doublings + 5 additions (the set bits of |x| below the top one)

#define TW __host__ __device__ static inline
#if defined(__HIP_DEVICE_COMPILE__)
#define TW_NI __host__ __device__ static __noinline__
#else
#define TW_NI __host__ __device__ static inline
#endif

TW Fp fz() { return zero<FpParams>(); }
TW Fp fo() { return one<FpParams>(); }

// ---------------- Fp2 ----------------
TW Fp2 operator+(const Fp2& a, const Fp2& b) { return {add(a.c0, b.c0), add(a.c1, b.c1)}; }
TW Fp2 operator-(const Fp2& a, const Fp2& b) { return {sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
TW Fp2 neg2(const Fp2& a) { return {neg(a.c0), neg(a.c1)}; }
TW Fp2 conj(const Fp2& a) { return {a.c0, neg(a.c1)}; }
// (device: operands by value, i.e. in registers; a reference would send them through scratch memory)
TW_NI Fp2 mul2(const Fp2 a, const Fp2 b) {  // Karatsuba, 3 Fp mul
    Fp t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1);
    Fp t2 = mul(add(a.c0, a.c1), add(b.c0, b.c1));
    return {sub(t0, t1), sub(sub(t2, t0), t1)};
}
TW Fp2 operator*(const Fp2& a, const Fp2& b) { return mul2(a, b); }
TW_NI Fp2 sqr2(const Fp2 a) {  // (a0+a1)(a0-a1), 2 a0 a1
    Fp t = mul(a.c0, a.c1);
    return {mul(add(a.c0, a.c1), sub(a.c0, a.c1)), add(t, t)};
}
TW_NI Fp2 scale(const Fp2 a, const Fp s) { return {mul(a.c0, s), mul(a.c1, s)}; }
TW Fp2 mul_xi(const Fp2& a) { return {sub(a.c0, a.c1), add(a.c0, a.c1)}; }  // * (1+u)
TW_NI Fp inv_fp(const Fp a) { return inv(a); }
TW Fp2 inv2(const Fp2& a) {
    Fp n = inv_fp(add(sqr(a.c0), sqr(a.c1)));
    const Fp2 s = scale(a, n);
    return {s.c0, neg(s.c1)};
}
TW bool is_zero2(const Fp2& a) { return is_zero(a.c0) && is_zero(a.c1); }
TW bool eq2(const Fp2& a, const Fp2& b) { return eq(a.c0, b.c0) && eq(a.c1, b.c1); }
TW Fp2 zero2() { return {fz(), fz()}; }
TW Fp2 one2() { return {fo(), fz()}; }

// ---------------- Fp6 ----------------
TW Fp6 operator+(const Fp6& a, const Fp6& b) { return {a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2}; }
TW Fp6 operator-(const Fp6& a, const Fp6& b) { return {a.c0 - b.c0, a.c1 - b.c1, a.c2 - b.c2}; }
TW Fp6 neg6(const Fp6& a) { return {neg2(a.c0), neg2(a.c1), neg2(a.c2)}; }
TW_NI Fp6 mul6(const Fp6& a, const Fp6& b) {  // Karatsuba-style, 6 Fp2 mul
    Fp2 v0 = a.c0 * b.c0, v1 = a.c1 * b.c1, v2 = a.c2 * b.c2;
    Fp2 c0 = v0 + mul_xi((a.c1 + a.c2) * (b.c1 + b.c2) - v1 - v2);
    Fp2 c1 = (a.c0 + a.c1) * (b.c0 + b.c1) - v0 - v1 + mul_xi(v2);
    Fp2 c2 = (a.c0 + a.c2) * (b.c0 + b.c2) - v0 - v2 + v1;
    return {c0, c1, c2};
}
TW Fp6 operator*(const Fp6& a, const Fp6& b) { return mul6(a, b); }
TW Fp6 mul_v(const Fp6& a) { return {mul_xi(a.c2), a.c0, a.c1}; }
TW Fp6 inv6(const Fp6& a) {
    Fp2 t0 = sqr2(a.c0) - mul_xi(a.c1 * a.c2);
    Fp2 t1 = mul_xi(sqr2(a.c2)) - a.c0 * a.c1;
    Fp2 t2 = sqr2(a.c1) - a.c0 * a.c2;
    Fp2 d = inv2(a.c0 * t0 + mul_xi(a.c2 * t1 + a.c1 * t2));
    return {t0 * d, t1 * d, t2 * d};
}

// ---------------- Fp12 ----------------
TW Fp12 one12() { return {{one2(), zero2(), zero2()}, {zero2(), zero2(), zero2()}}; }
TW_NI Fp12 mul12(const Fp12& a, const Fp12& b) {  // 3 Fp6 mul
    Fp6 v0 = a.c0 * b.c0, v1 = a.c1 * b.c1;
    Fp6 c1 = (a.c0 + a.c1) * (b.c0 + b.c1) - v0 - v1;
    return {v0 + mul_v(v1), c1};
}
TW Fp12 operator*(const Fp12& a, const Fp12& b) { return mul12(a, b); }
// a^2 by the complex method: (a0 + a1 w)^2 = (a0 + a1)(a0 + v a1) - t - v t + 2 t w, t = a0 a1: 2 Fp6 multiplications instead of 3
TW_NI Fp12 sqr12(const Fp12& a) {
    const Fp6 t = a.c0 * a.c1;
    const Fp6 c0 = (a.c0 + a.c1) * (a.c0 + mul_v(a.c1)) - t - mul_v(t);
    return {c0, t + t};
}
// (x0 + x1 v + x2 v^2)(A + B v): 5 Fp2 multiplications
TW_NI Fp6 mul6_by_01(const Fp6& x, const Fp2& A, const Fp2& B) {
    const Fp2 aa = x.c0 * A, bb = x.c1 * B;
    const Fp2 c0 = mul_xi((x.c1 + x.c2) * B - bb) + aa;
    const Fp2 c2 = (x.c0 + x.c2) * A - aa + bb;
    const Fp2 c1 = (x.c0 + x.c1) * (A + B) - aa - bb;
    return {c0, c1, c2};
}
// (x0 + x1 v + x2 v^2)(y v), y in Fp: (xi x2 y, x0 y, x1 y)
TW Fp6 mul6_by_1fp(const Fp6& x, const Fp& y) { return {mul_xi(scale(x.c2, y)), scale(x.c0, y), scale(x.c1, y)}; }
// f * (A + B v + y v w): the value of a line at a G1 point has three of its six Fp2 coefficients, one of them in Fp.
// Karatsuba over w with the sparse factors: 5 + 5 Fp2 multiplications + 6 by an Fp, against 18 for a general product.
TW_NI Fp12 mul12_by_line(const Fp12& f, const Fp2& A, const Fp2& B, const Fp& y) {
    const Fp6 v0 = mul6_by_01(f.c0, A, B), v1 = mul6_by_1fp(f.c1, y);
    const Fp2 By = {add(B.c0, y), B.c1};
    const Fp6 c1 = mul6_by_01(f.c0 + f.c1, A, By) - v0 - v1;
    return {v0 + mul_v(v1), c1};
}
// (x + y s)^2, s^2 = xi
TW void fp4_sqr(const Fp2& x, const Fp2& y, Fp2& s0, Fp2& s1) {
    const Fp2 t = x * y;
    s0 = (x + y) * (mul_xi(y) + x) - t - mul_xi(t);
    s1 = t + t;
}
TW Fp2 three_minus_two(const Fp2& t, const Fp2& z) { Fp2 d = t - z; return d + d + t; }  // 3 t - 2 z
TW Fp2 three_plus_two(const Fp2& t, const Fp2& z) { Fp2 d = t + z; return d + d + t; }    // 3 t + 2 z
// a^2 for a in the cyclotomic subgroup (a^(p^6+1) = 1, where every value sits after the easy part of the final
// exponentiation): Granger-Scott squaring, three Fp4 squarings = 6 Fp2 multiplications instead of 18.
TW_NI Fp12 cyc_sqr12(const Fp12& a) {
    const Fp2 &r0 = a.c0.c0, &r4 = a.c0.c1, &r3 = a.c0.c2, &r2 = a.c1.c0, &r1 = a.c1.c1, &r5 = a.c1.c2;
    Fp2 t0, t1, t2, t3, t4, t5;
    fp4_sqr(r0, r1, t0, t1);
    fp4_sqr(r2, r3, t2, t3);
    fp4_sqr(r4, r5, t4, t5);
    Fp12 r;
    r.c0.c0 = three_minus_two(t0, r0);
    r.c1.c1 = three_plus_two(t1, r1);
    r.c1.c0 = three_plus_two(mul_xi(t5), r2);
    r.c0.c2 = three_minus_two(t4, r3);
    r.c0.c1 = three_minus_two(t2, r4);
    r.c1.c2 = three_plus_two(t3, r5);
    return r;
}
TW Fp12 conj12(const Fp12& a) { return {a.c0, neg6(a.c1)}; }
TW_NI Fp12 inv12(const Fp12& a) {
    Fp6 t = inv6(a.c0 * a.c0 - mul_v(a.c1 * a.c1));
    return {a.c0 * t, neg6(a.c1 * t)};
}
TW bool is_one12(const Fp12& a) {
    const Fp2* x = &a.c0.c0;
    bool ok = eq2(x[0], one2());
    for (int i = 1; i < 6; i++) ok = ok && is_zero2(x[i]);
    return ok;
}
TW Fp6 frob6(const Fp6& a, const FrobConsts& fc) { return {conj(a.c0), conj(a.c1) * fc.g2, conj(a.c2) * fc.g4}; }
TW_NI Fp12 frob12(const Fp12& a, const FrobConsts& fc) {
    Fp6 c1 = frob6(a.c1, fc);
    return {frob6(a.c0, fc), {c1.c0 * fc.g1, c1.c1 * fc.g1, c1.c2 * fc.g1}};
}

TW_NI Fp12 pow_x(const Fp12& f) {  // f^x with x negative: conj(f^|x|) inside the cyclotomic subgroup
    Fp12 acc = f;
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        acc = cyc_sqr12(acc);
        if ((X_ABS >> i) & 1) acc = acc * f;
    }
    return conj12(acc);
}

// prod_k (the Miller value of P[k] against the prepared lines[k]), conjugated (x < 0).  A pair with skip[k] set (an identity on
// either side) contributes 1.  On the device that is a SELECT after the product, not a branch around it: the loop over the bits of
// |x| stays uniform across the wave, whichever lanes hold an identity.  The host skips the product.
TW Fp12 miller_loop_lines(const G1Affine* P, const Line* const* lines, const bool* skip, int n) {
    Fp12 f = one12();
    int idx = 0;
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        f = sqr12(f);
        const int steps = ((X_ABS >> i) & 1) ? 2 : 1;
#pragma unroll 1
        for (int s = 0; s < steps; s++, idx++)
#pragma unroll 1
            for (int k = 0; k < n; k++) {
#if defined(__HIP_DEVICE_COMPILE__)
                const Line& l = lines[k][idx];
                const Fp12 g = mul12_by_line(f, l.a, scale(l.b, P[k].x), P[k].y);
                uint32_t* fw = (uint32_t*)&f;
                const uint32_t* gw = (const uint32_t*)&g;
                for (int w = 0; w < (int)(sizeof(Fp12) / 4); w++) fw[w] = skip[k] ? fw[w] : gw[w];
#else
                if (skip[k]) continue;
                const Line& l = lines[k][idx];
                f = mul12_by_line(f, l.a, scale(l.b, P[k].x), P[k].y);
#endif
            }
    }
    return conj12(f);  // x < 0
}

TW bool final_exponentiation_is_one(const Fp12& f, const FrobConsts& fc) {
    // easy part: f^((p^6-1)(p^2+1))
    Fp12 t = conj12(f) * inv12(f);
    t = frob12(frob12(t, fc), fc) * t;
    // hard part, up to the harmless factor 3: 3(p^4-p^2+1)/r = (x-1)^2 (x+p)(x^2+p^2-1) + 3
    Fp12 a = pow_x(t) * conj12(t);            // t^(x-1)
    a = pow_x(a) * conj12(a);                 // t^((x-1)^2)
    Fp12 b = pow_x(a) * frob12(a, fc);        // ^(x+p)
    Fp12 c = pow_x(pow_x(b)) * frob12(frob12(b, fc), fc) * conj12(b);  // ^(x^2+p^2-1)
    Fp12 r = c * (t * t * t);
    return is_one12(r);
}

// ---------------- one check, as a lane of k_pairing_check runs it ----------------
// the 0xff poison of the many-verifications' result slots, still there: the device never wrote that sum
TW bool poisoned(const JacQ& s) { return s.x.v[0] == 0xffffffffu && s.z.v[0] == 0xffffffffu; }
TW_NI G1Affine affine_of(const JacQ& p) { return to_affine(jac_from_jacq(p)); }
// e(two[0], key0) e(two[1], key1) == 1 ?  1 / 0, or -1 where an input is poisoned.  key0 / key1: MILLER_LINES prepared lines each
// (of G2 points that are not the identity).  miller (may be null) receives the Miller value before the final exponentiation.
TW int check_lane(const JacQ* two, const Line* key0, const Line* key1, const FrobConsts& fc, Fp12* miller) {
    if (poisoned(two[0]) || poisoned(two[1])) return -1;
    G1Affine P[2];
#pragma unroll 1
    for (int j = 0; j < 2; j++) P[j] = affine_of(two[j]);
    const Line* const lines[2] = {key0, key1};
    const bool skip[2] = {is_inf(P[0]), is_inf(P[1])};
    const Fp12 f = miller_loop_lines(P, lines, skip, 2);
    if (miller) *miller = f;
    return final_exponentiation_is_one(f, fc) ? 1 : 0;
}

}  // namespace pairing
}  // namespace kzg
