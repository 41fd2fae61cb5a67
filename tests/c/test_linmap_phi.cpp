// CPU check of the G1 endomorphism in the compiled linear map (csrc/g1_linmap.hpp: Toom-Cook points on the sixth roots of
// unity, rotations as operand modifiers; k_g1slp.hip applies them with curve30.hpp's apply_phi):
//   * phi(X : Y : Z) = (beta X : Y : Z) on the signed 13 x 30-bit points equals [lambda] P of the saturated group law for points
//     of the r-torsion, lambda the GLV constant the plans are compiled with and beta picked the way the engine picks it; also
//     phi^2 = [lambda^2], an addition with a rotated operand, and v + phi(v) = -phi^2(v) (the identity the plan builder folds);
//   * every strategy's plan and each of its four schedule forms equal the map's definition over Fr, and the Hankel products on
//     the mu_6 points for every size and split (4, 8, 16);
//   * the operation counts and priced cost of the tuned plans with and without phi are printed.
// Built and run by tests/test_linmap_phi.py with hipcc's host pass (no kernel is launched).
#include "curve30.hpp"
#include "g1_linmap.hpp"
#include <cstdio>
using namespace kzg;
using namespace kzg::linmap;

static uint64_t st = 0x13198a2e03707344ull;
static uint32_t rnd() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 11); }
static Fr rnd_fr() {
    Fr a;
    for (int i = 0; i < 8; i++) a.v[i] = rnd();
    a.v[7] &= 0x3fffffffu;
    return a;
}
static Fr fr_pow(Fr b, const uint32_t* e, int nl) {
    Fr acc = one<FrParams>();
    for (int i = 32 * nl - 1; i >= 0; i--) { acc = sqr(acc); if ((e[i >> 5] >> (i & 31)) & 1) acc = mul(acc, b); }
    return acc;
}
static G1Affine random_point() {  // on y^2 = x^3 + 4
    for (;;) {
        Fp x;
        for (int i = 0; i < 12; i++) x.v[i] = rnd();
        x.v[11] &= 0x0fffffffu;
        Fp four = zero<FpParams>();
        four.v[0] = 4;
        Fp rhs = add(mul(sqr(x), x), to_mont(four)), y;
        if (fp_sqrt(y, rhs)) { G1Affine a; a.x = x; a.y = (rnd() & 1) ? y : neg(y); return a; }
    }
}
static const uint32_t H_EFF[2] = {0x00010001u, 0xd2010000u};                          // 1 - z: clears the cofactor of G1
static const uint32_t LAMBDA[4] = {0xffffffffu, 0x00000000u, 0x0001a402u, 0xac45a401u};  // the GLV lambda (engine.hip: GLV_LAMBDA)
static G1Jac random_g1() { return scalar_mul<2>(to_jac(random_point()), H_EFF); }
static G1Jac jac_from_jacs(const JacS& p) {
    if (is_inf(p)) return jac_inf();
    G1Jac r;
    r.x = fp_from_fs(p.x);
    r.y = fp_from_fs(p.y);
    r.z = fp_from_fs(p.z);
    return r;
}
static int bad = 0;
static void expect(const JacS& got, const G1Jac& want, const char* what) {
    if (!eq(jac_from_jacs(got), want)) { bad++; if (bad < 10) printf("MISMATCH %s\n", what); }
}

static void check_phi() {
    // beta as the engine picks it (engine.hip: init_srs): x([lambda] P) / x(P) on a point of G1
    G1Jac P0 = random_g1();
    const G1Affine a = to_affine(P0), la = to_affine(scalar_mul<4>(P0, LAMBDA));
    const Fp beta = mul(la.x, inv(a.x));
    if (!eq(mul(sqr(beta), beta), one<FpParams>()) || eq(beta, one<FpParams>()) || !eq(la.y, a.y)) { bad++; printf("beta: not the endomorphism\n"); return; }
    {   // the lambda of the plans is that GLV lambda
        Fr lam = zero<FrParams>();
        for (int i = 0; i < 4; i++) lam.v[i] = LAMBDA[i];
        if (!eq(to_mont(lam), glv_lambda())) { bad++; printf("glv_lambda() differs from the GLV constant\n"); }
    }
    const Fs<1, DC> bs = fs_from_fp(beta);
    int n = 0;
    for (int it = 0; it < 60; it++) {
        G1Jac P = random_g1(), Q = random_g1();
        for (int k = 0; k < (it % 4); k++) { P = dbl(P); Q = add(Q, P); }  // non-trivial Z
        const JacS p = jacs_from_jacq(jacq_from_jac(P)), q = jacs_from_jacq(jacq_from_jac(Q));
        const G1Jac lP = scalar_mul<4>(P, LAMBDA), llP = scalar_mul<4>(lP, LAMBDA), lQ = scalar_mul<4>(Q, LAMBDA), llQ = scalar_mul<4>(lQ, LAMBDA);
        expect(apply_phi(p, bs), lP, "phi = [lambda]");
        expect(apply_phi(apply_phi(p, bs), bs), llP, "phi^2 = [lambda^2]");
        expect(add(p, apply_phi(q, bs)), add(P, lQ), "P + phi(Q)");
        expect(add(p, apply_phi(apply_phi(q, bs), bs), true), add(P, neg(llQ)), "P - phi^2(Q)");
        expect(add(p, apply_phi(p, bs)), neg(llP), "P + phi(P) = -phi^2(P)");
        {
            JacS s, d;
            add_sub(dbl_half(apply_phi(p, bs)), apply_phi(q, bs), s, d);
            expect(s, add(dbl(lP), lQ), "pair sum, rotated operands");
            expect(d, add(dbl(lP), neg(lQ)), "pair difference, rotated operands");
        }
        bool deg = false;
        const JacS u = add_unchecked(apply_phi(p, bs), q, false, deg);
        if (!deg) expect(u, add(lP, Q), "add_unchecked phi(P) + Q");
        expect(apply_phi(jacs_inf(), bs), jac_inf(), "phi(O)");
        n += 9;
    }
    printf("phi on JacS: %d checks\n", n);
}

int main() {
    check_phi();
    uint32_t e[8];
    for (int i = 0; i < 8; i++) e[i] = FrParams::MOD[i];
    e[0] -= 1;
    for (int s = 0; s < 7; s++) for (int i = 0; i < 8; i++) e[i] = (e[i] >> 1) | (i < 7 ? (e[i + 1] << 31) : 0);
    const Fr g = fr_pow(fr_small(7), e, 8);
    std::vector<Fr> w(128);
    w[0] = one<FrParams>();
    for (int i = 1; i < 128; i++) w[i] = mul(w[i - 1], g);

    // Hankel products on the mu_6 points
    for (int k : {4, 8, 16})
        for (int n : {4, 8, 16, 32}) {
            if (n % k) continue;
            Compiler C;
            C.phi = true;
            C.tune(32);
            C.hankel_split[n] = k;
            Builder B(n);
            std::vector<Ref> x(n);
            for (int i = 0; i < n; i++) x[i] = B.input(i);
            std::vector<Fr> h(2 * n - 1), in(n);
            for (auto& v : h) v = rnd_fr();
            for (auto& v : in) v = rnd_fr();
            const auto y = C.hankel(B, x, h);
            const Plan p = B.take(y);
            const auto got = run_over_fr(p, in);
            for (int i = 0; i < n; i++) {
                Fr acc = zero<FrParams>();
                for (int j = 0; j < n; j++) acc = add(acc, mul(h[i + j], in[j]));
                if (!eq(acc, got[i])) { bad++; if (bad < 10) printf("MISMATCH mu6 hankel n=%d k=%d i=%d\n", n, k, i); }
            }
            printf("mu6 hankel n=%2d split %2d: %4ld mulc %5ld add %5ld dbl %4ld phi\n", n, k, p.count(OP_MULC), p.count(OP_ADD) + p.count(OP_SUB),
                   p.doublings(), p.rotations());
        }

    // every strategy: the engine's (tuned with phi; the four fixed small-batch ones without) and more, plan and all schedule forms
    struct S_ { bool tuned, phi, balanced; int k4, k8, k16, k32; };
    const S_ strategies[] = {{true, true, false, 0, 0, 0, 0},    {true, false, false, 0, 0, 0, 0},  {false, false, true, 2, 2, 2, 2},
                             {false, false, true, 4, 2, 4, 2},   {false, false, true, 2, 2, 2, 4},  {false, false, true, 4, 2, 4, 8},
                             {false, true, true, 4, 2, 4, 8},    {false, true, true, 4, 8, 16, 16}, {false, true, false, 4, 4, 16, 16},
                             {false, true, true, 2, 2, 2, 2}};
    for (auto& sd : strategies) {
        Strategy s;
        s.tuned = sd.tuned;
        s.phi = sd.phi;
        s.balanced_lincomb = sd.balanced;
        if (!sd.tuned) s.hankel_split = {{2, 2}, {4, sd.k4}, {8, sd.k8}, {16, sd.k16}, {32, sd.k32}};
        const Plan p = build_fk20_proofs_plan(w, s);
        printf("strategy tuned=%d phi=%d splits %d %d %d %d: %ld mulc, %ld add/sub, %ld doublings, %ld phi operands, cost %.1f M\n", sd.tuned, sd.phi,
               sd.k4, sd.k8, sd.k16, sd.k32, p.count(OP_MULC), p.count(OP_ADD) + p.count(OP_SUB), p.doublings(), p.rotations(), Builder::plan_cost(p) / 1e6);
        for (int it = 0; it < 3; it++) {
            std::vector<Fr> in(128);
            for (auto& v : in) v = rnd_fr();
            if (it == 1) for (auto& v : in) v = zero<FrParams>();
            if (it == 2) for (int j = 0; j < 128; j++) in[j] = j == 93 ? one<FrParams>() : zero<FrParams>();
            const auto want = fk20_proofs_map_by_definition(w, in);
            const auto got = run_over_fr(p, in);
            for (int k = 0; k < 128; k++)
                if (!eq(want[k], got[k])) { bad++; if (bad < 10) printf("MISMATCH plan out %d\n", k); }
            for (int form = 0; form < 4; form++) {
                const Schedule F = make_schedule(p, (form & 1) != 0, (form & 2) != 0);
                const auto got2 = run_schedule_over_fr(F, p.consts, 128, 128, in);
                for (int k = 0; k < 128; k++)
                    if (!eq(want[k], got2[k])) { bad++; if (bad < 10) printf("MISMATCH schedule form %d out %d\n", form, k); }
                for (size_t i = 3; i < F.words.size(); i += 4)  // a rotation field is 0, 1 or 2
                    if ((F.words[i] & 3u) != 2u && (((F.words[i] >> 8) & 3u) == 3u || ((F.words[i] >> 10) & 3u) == 3u)) { bad++; printf("bad rotation word\n"); break; }
            }
        }
    }
    printf("%d mismatches\n", bad);
    return bad != 0;
}
