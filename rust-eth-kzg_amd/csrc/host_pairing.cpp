// See host_pairing.hpp.  Tower Fp2 = Fp[u]/(u^2+1), Fp6 = Fp2[v]/(v^3-(1+u)), Fp12 = Fp6[w]/(w^2-v);
// M-type twist E'(Fp2): y^2 = x^3 + 4(1+u), untwist (x, y) -> (x / w^2, y / w^3).
#include "host_pairing.hpp"
#include <mutex>

namespace kzg {
namespace pairing {

using FpP = FpParams;

// ---------------- Fp2 (arithmetic: pairing_tower.hpp) ----------------
static Fp2 pow2(const Fp2& a, const uint32_t* e, int nl) {
    Fp2 acc = one2();
    for (int i = 32 * nl - 1; i >= 0; i--) {
        acc = sqr2(acc);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = acc * a;
    }
    return acc;
}
static bool sqrt2(Fp2& out, const Fp2& a) {  // p = 3 mod 4 (Adj & Rodriguez-Henriquez, Alg. 9)
    static const uint32_t E1[12] = {0xffffeaaau, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                                    0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};  // (p-3)/4
    static const uint32_t E2[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u,
                                    0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};  // (p-1)/2
    if (is_zero2(a)) { out = a; return true; }
    Fp2 a1 = pow2(a, E1, 12);
    Fp2 x0 = a1 * a;
    Fp2 alpha = a1 * x0;
    Fp2 a0 = conj(alpha) * alpha;
    Fp2 m1 = {neg(fo()), fz()};
    if (eq2(a0, m1)) return false;
    Fp2 x;
    if (eq2(alpha, m1)) x = {neg(x0.c1), x0.c0};  // u * x0
    else {
        Fp2 t = alpha;
        t.c0 = add(t.c0, fo());
        x = pow2(t, E2, 12) * x0;
    }
    if (!eq2(sqr2(x), a)) return false;
    out = x;
    return true;
}

// Frobenius: v^p = xi^((p-1)/3) v, w^p = xi^((p-1)/6) w
static FrobConsts FC;  // xi^((p-1)/6), its square, its fourth power
static void init_once();
void init() {  // contexts are created from any thread, and the engines of a device list side by side (c_api.cpp): once, with a fence
    static std::once_flag once;
    std::call_once(once, init_once);
}
static void init_once() {
    static const uint32_t P16[12] = {0xfffff1c7u, 0x49aa7fffu, 0x72e35555u, 0x051caaaau, 0xd3c82906u, 0xe688231au,
                                     0x7deb831fu, 0xe613e1ebu, 0xb5e1f223u, 0x0c849bf3u, 0x5eeaa66fu, 0x045582fcu};  // (p-1)/6
    Fp2 xi = {fo(), fo()};
    FC.g1 = pow2(xi, P16, 12);
    FC.g2 = sqr2(FC.g1);
    FC.g4 = sqr2(FC.g2);
}
const FrobConsts& frob_consts() {
    init();
    return FC;
}
static inline Fp12 frob12(const Fp12& a) { return frob12(a, FC); }  // (after init)

// ---------------- G2 ----------------
static bool lex_largest2(const Fp2& y) { return is_zero(y.c1) ? fp_is_lex_largest(y.c0) : fp_is_lex_largest(y.c1); }
static bool fp_from_be48(Fp& out, const uint8_t* in, bool mask_flags) {
    Fp x;
    for (int i = 0; i < 12; i++) {
        uint32_t w = ((uint32_t)in[4 * i] << 24) | ((uint32_t)in[4 * i + 1] << 16) | ((uint32_t)in[4 * i + 2] << 8) | in[4 * i + 3];
        if (i == 0 && mask_flags) w &= 0x1fffffffu;
        x.v[11 - i] = w;
    }
    if (geq_mod<FpP>(x.v)) return false;
    out = to_mont(x);
    return true;
}
bool g2_decompress(G2Affine& out, const uint8_t in[96]) {
    bool compressed = (in[0] >> 7) & 1, infinity = (in[0] >> 6) & 1, sign = (in[0] >> 5) & 1;
    if (!compressed) return false;
    Fp2 x;
    if (!fp_from_be48(x.c1, in, true) || !fp_from_be48(x.c0, in + 48, false)) return false;
    if (infinity) {
        if (sign || !is_zero2(x)) return false;
        out = {zero2(), zero2(), true};
        return true;
    }
    Fp four = zero<FpP>();
    four.v[0] = 4;
    four = to_mont(four);
    Fp2 y2 = sqr2(x) * x + Fp2{four, four}, y;
    if (!sqrt2(y, y2)) return false;
    if (lex_largest2(y) != sign) y = neg2(y);
    out = {x, y, false};
    return true;
}
G2Affine g2_neg(const G2Affine& q) { return {q.x, neg2(q.y), q.inf}; }

G2Prepared prepare(const G2Affine& q) {
    G2Prepared pr;
    pr.inf = q.inf;
    if (q.inf) return pr;
    Fp2 tx = q.x, ty = q.y;
    auto step = [&](bool dbl) {
        Fp2 lam;
        if (dbl) {
            Fp2 x2 = sqr2(tx);
            lam = (x2 + x2 + x2) * inv2(ty + ty);
        } else lam = (q.y - ty) * inv2(q.x - tx);
        pr.lines.push_back({lam * tx - ty, neg2(lam)});
        Fp2 x3 = sqr2(lam) - tx - (dbl ? tx : q.x);
        Fp2 y3 = lam * (tx - x3) - ty;
        tx = x3;
        ty = y3;
    };
    for (int i = 62; i >= 0; i--) {
        step(true);
        if ((X_ABS >> i) & 1) step(false);
    }
    return pr;
}

// the Miller loop and the final exponentiation: pairing_tower.hpp
static Fp12 miller_loop_n(const G1Affine* P, const G2Prepared* const* Q, int n) {
    std::vector<const Line*> lines((size_t)n);
    std::vector<char> skip((size_t)n);
    for (int k = 0; k < n; k++) {
        skip[(size_t)k] = is_inf(P[k]) || Q[k]->inf;
        lines[(size_t)k] = Q[k]->lines.data();
    }
    static_assert(sizeof(bool) == sizeof(char), "skip flags");
    return miller_loop_lines(P, lines.data(), (const bool*)skip.data(), n);
}
Fp12 miller_loop(const G1Affine& P, const G2Prepared& Q) {
    const G2Prepared* q = &Q;
    return miller_loop_n(&P, &q, 1);
}
Fp12 fp12_mul(const Fp12& a, const Fp12& b) { return a * b; }
bool product_is_one(const G1Affine* P, const G2Prepared* const* Q, int n) { return final_exponentiation_is_one(miller_loop_n(P, Q, n)); }
bool final_exponentiation_is_one(const Fp12& f) { return final_exponentiation_is_one(f, frob_consts()); }

// ---------------- G2 arithmetic for a caller-supplied setup ----------------
// Jacobian coordinates over Fp2 (a = 0); used once per setup, never per call.
struct G2Jac { Fp2 x, y, z; };
static inline G2Jac g2j_inf() { return {one2(), one2(), zero2()}; }
static inline G2Jac g2j_from(const G2Affine& a) { return a.inf ? g2j_inf() : G2Jac{a.x, a.y, one2()}; }
static G2Jac g2j_dbl(const G2Jac& p) {
    if (is_zero2(p.z)) return p;
    const Fp2 A = sqr2(p.x), B = sqr2(p.y), Cc = sqr2(B);
    Fp2 D = sqr2(p.x + B) - A - Cc;
    D = D + D;
    const Fp2 E = A + A + A, F = sqr2(E);
    G2Jac r;
    r.x = F - D - D;
    Fp2 c8 = Cc + Cc;
    c8 = c8 + c8;
    c8 = c8 + c8;
    r.y = E * (D - r.x) - c8;
    const Fp2 yz = p.y * p.z;
    r.z = yz + yz;
    return r;
}
static G2Jac g2j_add(const G2Jac& p, const G2Jac& q) {
    if (is_zero2(p.z)) return q;
    if (is_zero2(q.z)) return p;
    const Fp2 z1z1 = sqr2(p.z), z2z2 = sqr2(q.z);
    const Fp2 u1 = p.x * z2z2, u2 = q.x * z1z1;
    const Fp2 s1 = p.y * q.z * z2z2, s2 = q.y * p.z * z1z1;
    if (eq2(u1, u2)) return eq2(s1, s2) ? g2j_dbl(p) : g2j_inf();
    const Fp2 h = u2 - u1;
    Fp2 i = h + h;
    i = sqr2(i);
    const Fp2 j = h * i;
    Fp2 rr = s2 - s1;
    rr = rr + rr;
    const Fp2 v = u1 * i;
    G2Jac r;
    r.x = sqr2(rr) - j - v - v;
    Fp2 s1j = s1 * j;
    s1j = s1j + s1j;
    r.y = rr * (v - r.x) - s1j;
    r.z = (sqr2(p.z + q.z) - z1z1 - z2z2) * h;
    return r;
}
static bool g2j_eq(const G2Jac& p, const G2Jac& q) {
    const bool pi = is_zero2(p.z), qi = is_zero2(q.z);
    if (pi || qi) return pi && qi;
    const Fp2 z1z1 = sqr2(p.z), z2z2 = sqr2(q.z);
    return eq2(p.x * z2z2, q.x * z1z1) && eq2(p.y * q.z * z2z2, q.y * p.z * z1z1);
}
static G2Affine g2j_to_affine(const G2Jac& p) {
    if (is_zero2(p.z)) return {zero2(), zero2(), true};
    const Fp2 zi = inv2(p.z), zi2 = sqr2(zi);
    return {p.x * zi2, p.y * zi2 * zi, false};
}
static G2Jac g2j_mul(const G2Jac& p, const uint32_t* k, int nl) {
    G2Jac acc = g2j_inf();
    for (int i = 32 * nl - 1; i >= 0; i--) {
        acc = g2j_dbl(acc);
        if ((k[i >> 5] >> (i & 31)) & 1) acc = g2j_add(acc, p);
    }
    return acc;
}
bool g2_eq(const G2Affine& a, const G2Affine& b) {
    if (a.inf || b.inf) return a.inf && b.inf;
    return eq2(a.x, b.x) && eq2(a.y, b.y);
}
bool g2_killed_by_r(const G2Affine& q) { return is_zero2(g2j_mul(g2j_from(q), FrParams::MOD, 8).z); }
// psi = twist . Frobenius . untwist: (x, y) -> (conj(x) / xi^((p-1)/3), conj(y) / xi^((p-1)/2)); on E'(Fp2) the points of order r
// are exactly those with psi(Q) = [x]Q, x the (negative) BLS parameter (M. Scott, "A note on group membership tests for G1, G2
// and GT on BLS pairing-friendly curves", 2021): a 64-bit multiplication instead of the 255-bit one of the definition.
bool g2_in_subgroup(const G2Affine& q) {
    if (q.inf) return true;
    init();
    const Fp2 cx = inv2(FC.g2), cy = inv2(FC.g2 * FC.g1);
    const G2Jac psi = {conj(q.x) * cx, conj(q.y) * cy, one2()};
    const uint32_t xabs[2] = {(uint32_t)X_ABS, (uint32_t)(X_ABS >> 32)};
    G2Jac xq = g2j_mul(g2j_from(q), xabs, 2);
    xq.y = neg2(xq.y);  // x < 0
    return g2j_eq(psi, xq);
}
G2Affine g2_mul(const G2Affine& q, const uint32_t* k, int n_limbs) { return g2j_to_affine(g2j_mul(g2j_from(q), k, n_limbs)); }
G2Affine g2_lincomb128(const G2Affine* pts, const uint32_t (*k)[4], int n) {
    G2Jac acc = g2j_inf();
    std::vector<G2Jac> j((size_t)n);
    for (int i = 0; i < n; i++) j[(size_t)i] = g2j_from(pts[i]);
    for (int b = 127; b >= 0; b--) {  // the doublings are shared by all terms
        acc = g2j_dbl(acc);
        for (int i = 0; i < n; i++)
            if ((k[i][b >> 5] >> (b & 31)) & 1) acc = g2j_add(acc, j[(size_t)i]);
    }
    return g2j_to_affine(acc);
}
// x^3 + 4 (1 + u) as a curve point with the lexicographically smaller y, if it is a square (the tests' source of points off the subgroup)
bool g2_from_x(G2Affine& out, const Fp2& x) {
    Fp four = zero<FpP>();
    four.v[0] = 4;
    four = to_mont(four);
    Fp2 y;
    if (!sqrt2(y, sqr2(x) * x + Fp2{four, four})) return false;
    out = {x, y, false};
    return true;
}

}  // namespace pairing
}  // namespace kzg
