// CPU run of the FK20 tap of k_coeffs_to_cells_scalars (csrc/fr29_ntt.hpp, THE FK20 TAP): the forward network's radix-4 units on a
// random coefficient vector, both halves of the extended domain, stopped after the passes h = 1024, 256, 64; then the kernel's own tap
// (fk20_tap_scalar over the table fk20_tap_const builds, rows and columns from fk20_tap_row / fk20_tap_column).  The coefficients and
// all 8192 scalars are written out as plain integers; tests/test_fk20_tap_host.py evaluates the definition of the scalars on them in
// exact integers.  Built with hipcc's host pass: no kernel is launched.
#include "fr29.hpp"
#include "fr29_ntt.hpp"
#include <cstdio>
#include <vector>
using namespace kzg;

static uint64_t st = 0x243f6a8885a308d3ull;
static uint32_t rnd32() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 16); }
static Fr rnd_fr() {  // canonical value < r (as a plain integer)
    Fr a;
    for (int i = 0; i < 8; i++) a.v[i] = rnd32();
    a.v[7] &= 0x3fffffffu;
    return a;
}
static Fr small(uint32_t v) { Fr a = zero<FrParams>(); a.v[0] = v; return a; }
static Fr29 x_of(const Fr& y_mont) { return fr29_from_plain(mul(y_mont, to_mont(small(32)))); }  // the 9 x 29-bit Montgomery form
static void put(FILE* f, const char* tag, const Fr& plain) {
    fprintf(f, "%s ", tag);
    for (int i = 7; i >= 0; i--) fprintf(f, "%08x", plain.v[i]);
    fprintf(f, "\n");
}
struct VecElems {
    std::vector<Fr29>* v;
    Fr29 load(int i) const { return (*v)[i]; }
    void store(int i, const Fr29& x) const { (*v)[i] = x; }
};

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "w");
    if (!f) return 2;
    // omega_8192 = 7^((r - 1) / 8192) and its powers
    uint32_t e[8];
    for (int i = 0; i < 8; i++) e[i] = FrParams::MOD[i];
    e[0] -= 1;
    for (int s = 0; s < 13; s++) for (int i = 0; i < 8; i++) e[i] = (e[i] >> 1) | (i < 7 ? (e[i + 1] << 31) : 0);
    Fr g = one<FrParams>(), base = to_mont(small(7));
    for (int i = 255; i >= 0; i--) { g = sqr(g); if ((e[i >> 5] >> (i & 31)) & 1) g = mul(g, base); }
    std::vector<Fr29> w29(NTT_W);
    {
        Fr w = one<FrParams>();
        for (int i = 0; i < NTT_W; i++) { w29[i] = x_of(w); w = mul(w, g); }
    }
    put(f, "omega", from_mont(g));
    // the scale of linear-map mode, 1/2 = (r + 1) / 2, as a plain integer
    Fr half;
    for (int i = 0; i < 8; i++) half.v[i] = FrParams::MOD[i];
    half.v[0] += 1;
    for (int i = 0; i < 8; i++) half.v[i] = (half.v[i] >> 1) | (i < 7 ? (half.v[i + 1] << 31) : 0);
    put(f, "scale", half);
    std::vector<Fr29> tapk(2 * NTT_N);
    for (int idx = 0; idx < 2 * NTT_N; idx++) tapk[idx] = fk20_tap_const(w29.data(), fr29_from_plain(half), idx);
    // coefficients as the engine stores them (saturated Montgomery form), with the edges of every index class planted
    std::vector<Fr> a(NTT_N);
    for (auto& v : a) v = to_mont(rnd_fr());
    Fr top;
    for (int i = 0; i < 8; i++) top.v[i] = FrParams::MOD[i];
    top.v[0] -= 1;
    a[0] = to_mont(top);
    a[63] = zero<FrParams>();
    a[64] = to_mont(small(1));
    a[4095] = to_mont(top);
    for (int i = 0; i < NTT_N; i++) put(f, "a", from_mont(a[i]));
    int bad = 0;
    for (int h = 0; h < 2; h++) {
        std::vector<Fr29> x(NTT_N);
        for (int i = 0; i < NTT_N; i++) {  // the input stage of k_coeffs_to_cells_scalars
            Fr29 c = fr29_from_fr_mont(a[i]);
            if (h && i) c = fr29_mul(c, w29[i]);
            x[i] = c;
        }
        int log_m = 0;
        for (int hh = 1024; hh >= 64; hh >>= 2, log_m += 2)
            for (int u = 0; u < 1024; u++) ntt4096_ct_forward_unit(VecElems{&x}, w29.data(), hh, log_m, u);
        for (int i = 0; i < NTT_N; i++) {
            const Fr29 s = fk20_tap_scalar(VecElems{&x}, tapk.data(), i, h);
            for (int l = 0; l < RL - 1; l++) if (s.v[l] > RMASK) bad++;
            Fr plain;
            fr29_to_words(plain.v, fr29_reduce_once(s));
            fprintf(f, "s %d %d ", fk20_tap_row(i, h), fk20_tap_column(i));
            for (int k = 7; k >= 0; k--) fprintf(f, "%08x", plain.v[k]);
            fprintf(f, "\n");
        }
    }
    fclose(f);
    printf("%d mismatches\n", bad);
    return bad != 0;
}
