// CPU check of csrc/pairing_tower.hpp, the tower arithmetic the host's pairing checks and k_pairing_check share: check_lane -- what one
// lane of the kernel runs -- on pairs whose verdict is known BY CONSTRUCTION from the trusted setup's monomial points S_i = [tau^i]_1:
//   key 0 = ([tau^64]_2, -[1]_2), k = 64;  key 1 = ([tau]_2, -[1]_2), k = 1
//   (a S_i, a S_(i+k)) passes; (a S_i, b S_(i+k)) with b != a, the swapped pair and (a S_i, -a S_(i+k)) fail; (O, O) passes, (O, X) and
//   (X, O) fail; every pair also with each point multiplied through by a Z != 1; a poisoned slot gives -1
// against that construction, against product_is_one, and the Miller value against the host API's pieces (miller_loop, fp12_mul,
// final_exponentiation_is_one).  Built (plain and under ASan + UBSan) and run by tests/test_pairing_tower_host.py with the path of
// rust-eth-kzg_amd/data/trusted_setup_4096.bin.  Prints one line per case: "<key> <name> <rescale> want <w> lane <v> host <h> miller <0|1>".
#include <vector>
#include "host_pairing.cpp"
#include <cstdio>
#include <cstring>
using namespace kzg;
using namespace kzg::pairing;

static uint64_t st = 0x2545f4914f6cdd1dull;
static uint32_t rnd() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 16); }
static G1Affine times(const G1Affine& p, const uint32_t k[8]) { return to_affine(scalar_mul<8>(to_jac(p), k)); }
static JacQ as_jacq(const G1Affine& a, uint32_t z_word) {  // z_word 1: normalised
    G1Jac j = to_jac(a);
    if (z_word != 1 && !is_inf(a)) {
        Fp z = zero<FpParams>();
        z.v[0] = z_word;
        z = to_mont(z);
        const Fp z2 = sqr(z);
        j.x = mul(a.x, z2); j.y = mul(a.y, mul(z2, z)); j.z = z;
    }
    return jacq_from_jac(j);
}
static bool same12(const Fp12& a, const Fp12& b) { return memcmp(&a, &b, sizeof(Fp12)) == 0; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    std::vector<uint8_t> srs(16 + 4096 * 48 + 65 * 96);
    if (fread(srs.data(), 1, srs.size(), fh) != srs.size() || memcmp(srs.data(), "KZGSRS01", 8)) return 2;
    fclose(fh);
    const uint8_t *g1 = srs.data() + 16, *g2 = g1 + 4096 * 48;
    G2Affine gen2, tau2, tau64;
    if (!g2_decompress(gen2, g2) || !g2_decompress(tau2, g2 + 96) || !g2_decompress(tau64, g2 + 96 * 64)) return 3;
    const G2Prepared q_neg = prepare(g2_neg(gen2)), q_tau = prepare(tau2), q_tau64 = prepare(tau64);
    if ((int)q_neg.lines.size() != MILLER_LINES || (int)q_tau.lines.size() != MILLER_LINES || (int)q_tau64.lines.size() != MILLER_LINES) return 3;
    const FrobConsts& fc = frob_consts();
    int bad = 0, cases = 0;
    for (int key = 0; key < 2; key++) {
        const int k = key ? 1 : 64;
        const G2Prepared* vk[2] = {key ? &q_tau : &q_tau64, &q_neg};
        for (int it = 0; it < 3; it++) {
            const int i = it == 0 ? 0 : it == 1 ? 4095 - k : (int)(rnd() % (4096 - k));
            G1Affine Si, Sk;
            if (g1_decompress(Si, g1 + 48 * (size_t)i) || g1_decompress(Sk, g1 + 48 * (size_t)(i + k))) return 3;
            uint32_t a[8], b[8];
            for (int w = 0; w < 8; w++) { a[w] = it ? rnd() : (w == 0); b[w] = rnd(); }
            a[7] &= 0x3fffffffu; b[7] &= 0x3fffffffu;
            const G1Affine aSi = times(Si, a), aSk = times(Sk, a), bSk = times(Sk, b), O = aff_inf();
            struct Case { const char* name; G1Affine p0, p1; int want; };
            const Case list[] = {{"valid", aSi, aSk, 1}, {"other_scalar", aSi, bSk, 0}, {"swapped", aSk, aSi, 0}, {"negated", aSi, neg(aSk), 0},
                                 {"O_O", O, O, 1},       {"O_X", O, aSk, 0},            {"X_O", aSi, O, 0}};
            for (const Case& c : list)
                for (int rescale = 0; rescale < 2; rescale++) {
                    const JacQ two[2] = {as_jacq(c.p0, rescale ? 2 + (uint32_t)cases : 1), as_jacq(c.p1, rescale ? 0x80000001u + (uint32_t)cases : 1)};
                    Fp12 f;
                    const int lane = check_lane(two, vk[0]->lines.data(), vk[1]->lines.data(), fc, &f);
                    const G1Affine P[2] = {c.p0, c.p1};
                    const int host = product_is_one(P, vk, 2) ? 1 : 0;
                    // the Miller value: the product of the two single loops of the host API, and its verdict by the host API
                    const Fp12 pieces = fp12_mul(miller_loop(c.p0, *vk[0]), miller_loop(c.p1, *vk[1]));
                    const bool miller_ok = same12(f, pieces) && (final_exponentiation_is_one(f, fc) ? 1 : 0) == host &&
                                           (final_exponentiation_is_one(pieces) ? 1 : 0) == host;
                    printf("%d %s %d want %d lane %d host %d miller %d\n", key, c.name, rescale, c.want, lane, host, miller_ok ? 1 : 0);
                    if (lane != c.want || host != c.want || !miller_ok) bad++;
                    cases++;
                }
            // a slot that still holds the result slots' poison: -1, whichever slot
            for (int slot = 0; slot < 2; slot++) {
                JacQ two[2] = {as_jacq(aSi, 1), as_jacq(aSk, 1)};
                memset(&two[slot], 0xff, sizeof(JacQ));
                const int lane = check_lane(two, vk[0]->lines.data(), vk[1]->lines.data(), fc, nullptr);
                printf("%d poison_%d 0 want -1 lane %d host -1 miller 1\n", key, slot, lane);
                if (lane != -1) bad++;
                cases++;
            }
        }
    }
    printf("pairing tower: %d cases, %d mismatches\n", cases, bad);
    return bad != 0;
}
