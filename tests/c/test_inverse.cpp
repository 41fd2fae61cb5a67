// CPU check of csrc/inverse.hpp (binary-GCD inversion) against Fermat's a^(p-2) from csrc/field.hpp.
// Built and run by tests/test_host_units.py:  hipcc -x hip --offload-arch=gfx950 (host pass only; no kernel is launched).
// Values come from the WHOLE field [1, m): a draw of BITS bits minus m once if it is >= m (2^BITS < 2 m for both fields), so that
// [2^254, r) and [2^380, p) -- 45 % of Fr, 38 % of Fp -- are inverted too; then the named edges.
#include "inverse.hpp"
#include <cstdio>
#include <cstdlib>
using namespace kzg;

template <class P>
static int check(const Felt<P>& a) {
    Felt<P> x = inv(a), y = inv_fast(a);
    return (!eq(x, y) || !eq(mul(a, y), one<P>())) ? 1 : 0;
}
template <class P>
static int run(const char* name, int iters) {
    uint64_t st = 0x9e3779b97f4a7c15ull;
    auto next = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 16); };
    int bad = 0, high = 0, cases = 0;
    for (int it = 0; it < iters; it++) {
        Felt<P> a;
        for (int i = 0; i < P::N; i++) a.v[i] = next();
        if (it < 40) {  // small and structured values first
            for (int i = 0; i < P::N; i++) a.v[i] = 0;
            a.v[0] = it + 1;
            if (it >= 20) a.v[(it - 20) % P::N] = 0x80000000u >> (it % 7);
            if (it == 39) for (int i = 0; i < P::N; i++) a.v[i] = P::MOD[i] - (i == 0);  // m - 1
        }
        if (P::BITS % 32) a.v[P::N - 1] &= (1u << (P::BITS % 32)) - 1;  // < 2^BITS < 2 m
        if (geq_mod<P>(a.v)) {
            uint32_t t[P::N];
            sub_limbs<P::N>(t, a.v, P::MOD);
            for (int i = 0; i < P::N; i++) a.v[i] = t[i];
        }
        if (is_zero(a)) continue;
        if ((a.v[P::N - 1] >> ((P::BITS - 1) % 32)) & 1) high++;
        bad += check<P>(a);
        cases++;
    }
    {   // 1, 2, m - 2, m - 1, (m - 1) / 2, (m + 1) / 2, 2^(BITS - 1)
        Felt<P> e[7];
        for (auto& x : e) x = zero<P>();
        e[0].v[0] = 1;
        e[1].v[0] = 2;
        sub_limbs<P::N>(e[2].v, P::MOD, e[1].v);  // (r's lowest word is 1: the subtraction borrows)
        sub_limbs<P::N>(e[3].v, P::MOD, e[0].v);
        for (int i = 0; i < P::N; i++) e[4].v[i] = (P::MOD[i] >> 1) | (i + 1 < P::N ? P::MOD[i + 1] << 31 : 0u);
        e[5] = e[4];
        for (int i = 0, c = 1; i < P::N && c; i++) { e[5].v[i] += 1; c = e[5].v[i] == 0; }
        e[6].v[(P::BITS - 1) / 32] = 1u << ((P::BITS - 1) % 32);
        if (geq_mod<P>(e[6].v)) bad++;
        for (const auto& x : e) { bad += check<P>(x); cases++; }
        {   // (m - 1) / 2 + (m + 1) / 2 == m
            uint32_t s[P::N];
            uint64_t c = 0;
            for (int i = 0; i < P::N; i++) { c += (uint64_t)e[4].v[i] + e[5].v[i]; s[i] = (uint32_t)c; c >>= 32; }
            for (int i = 0; i < P::N; i++) if (s[i] != P::MOD[i]) { bad++; break; }
        }
    }
    if (high < iters / 4) bad++;  // the upper part of the field is really drawn (expected: 45 % of Fr, 38 % of Fp)
    Felt<P> z = zero<P>();
    if (!is_zero(inv_fast(z))) bad++;
    printf("%s: %d cases (%d of them >= 2^%d), %d mismatches\n", name, cases, high, P::BITS - 1, bad);
    return bad;
}
int main() {
    int bad = run<FpParams>("Fp", 3000) + run<FrParams>("Fr", 3000);
    return bad ? 1 : 0;
}
