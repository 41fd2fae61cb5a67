// The six compilations of the FK20 proofs map the engine uploads (csrc/g1_linmap_programs.hpp), written out as JSON: per program
// the words (4 per operation), the launches as (kind, first, count), the number of arena slots and the constants as canonical
// big-endian Fr.  Nothing about the programs is stated here: the strategies, the order of the outputs and the form of the schedule
// come from the header the engine itself compiles them with.
// Built and run by tests/linmap_model.py with hipcc's host pass (no kernel is launched).
#include "g1_linmap_programs.hpp"
#include <cstdio>
using namespace kzg;
using namespace kzg::linmap;

static Fr fr_pow(Fr b, const uint32_t* e, int nl) {
    Fr acc = one<FrParams>();
    for (int i = 32 * nl - 1; i >= 0; i--) { acc = sqr(acc); if ((e[i >> 5] >> (i & 31)) & 1) acc = mul(acc, b); }
    return acc;
}
static void print_be(const Fr& mont) {
    const Fr x = from_mont(mont);
    for (int i = 7; i >= 0; i--) printf("%08x", x.v[i]);
}
int main() {
    // omega_128 = 7^((r-1)/128)
    uint32_t e[8];
    for (int i = 0; i < 8; i++) e[i] = FrParams::MOD[i];
    e[0] -= 1;
    for (int s = 0; s < 7; s++) for (int i = 0; i < 8; i++) e[i] = (e[i] >> 1) | (i < 7 ? (e[i + 1] << 31) : 0);
    const Fr g = fr_pow(fr_small(7), e, 8);
    std::vector<Fr> w(128);
    w[0] = one<FrParams>();
    for (int i = 1; i < 128; i++) w[i] = mul(w[i - 1], g);
    if (!eq(mul(w[127], g), one<FrParams>()) || eq(w[64], one<FrParams>())) { fprintf(stderr, "bad root of unity\n"); return 1; }

    printf("{\"lambda\": \"");
    print_be(glv_lambda());
    printf("\", \"omega128\": \"");
    print_be(g);
    printf("\", \"programs\": [\n");
    for (int id = 0; id < SLP_PROGRAM_COUNT; id++) {
        const SlpCompiled c = compile_slp_program(w, id);
        const Schedule& S = c.sched;
        printf("{\"id\": %d, \"n_slots\": %d, \"launches\": [", id, S.n_slots);
        for (size_t i = 0; i < S.launches.size(); i++)
            printf("%s[%d, %d, %d]", i ? ", " : "", (int)S.launches[i].kind, S.launches[i].first, S.launches[i].count);
        printf("],\n \"words\": [");
        for (size_t i = 0; i < S.words.size(); i++) printf("%s%u", i ? "," : "", S.words[i]);
        printf("],\n \"consts\": [");
        for (size_t i = 0; i < c.plan.consts.size(); i++) {
            printf("%s\"", i ? "," : "");
            print_be(c.plan.consts[i]);
            printf("\"");
        }
        printf("]}%s\n", id + 1 < SLP_PROGRAM_COUNT ? "," : "");
    }
    printf("]}\n");
    return 0;
}
