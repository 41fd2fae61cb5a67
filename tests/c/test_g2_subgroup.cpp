// CPU check of the G2 subgroup test a caller-supplied trusted setup goes through (csrc/host_pairing.cpp: g2_in_subgroup, the
// psi-endomorphism test) against the definition [r]Q = O (g2_killed_by_r):
//   multiples of the generator -- the setup's own [tau^i]_2 and small and 255-bit multiples of [1]_2 -- pass both;
//   curve points over small abscissas x = c + u, which lie in E'(Fp2) but (the cofactor is ~2^508) not in the subgroup, fail both;
//   the point at infinity passes (the reference's checked parser accepts it);
//   the sum of 128-bit multiples (g2_lincomb128, the structure check's G2 side) equals the sum of the single multiples.
// argv[1]: rust-eth-kzg_amd/data/trusted_setup_4096.bin; argv[2] (optional): a file of any multiple of 96 bytes, compressed points that
// must each decode to a curve point and FAIL both tests (the point tests/setup_material.py constructs in Python, and the points of
// small order and [k][1]_2 + small order of tests/small_order.py, which psi(Q) == [x]Q has to tell from the subgroup).
#include "host_pairing.cpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace kzg;
using namespace kzg::pairing;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    init();
    std::vector<uint8_t> file;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + n);
        fclose(f);
    }
    const uint8_t* g2 = file.data() + 16 + 4096 * 48;
    int bad = 0, on_subgroup = 0, off_subgroup = 0;
    std::vector<G2Affine> pts(65);
    for (int i = 0; i < 65; i++) {
        if (!g2_decompress(pts[i], g2 + 96 * i)) { printf("setup point %d does not decode\n", i); bad++; continue; }
        const bool fast = g2_in_subgroup(pts[i]), slow = i < 8 ? g2_killed_by_r(pts[i]) : true;
        if (!fast || !slow) { printf("setup point %d: psi test %d, [r]Q test %d\n", i, fast, slow); bad++; }
        on_subgroup++;
    }
    const G2Affine gen = pts[0];
    uint64_t st = 0x2545f4914f6cdd1dull;
    for (int t = 0; t < 12; t++) {  // k [1]_2: k = 1 .. 4, then random 255-bit k
        uint32_t k[8] = {0};
        if (t < 4) k[0] = (uint32_t)t + 1;
        else for (int i = 0; i < 8; i++) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; k[i] = (uint32_t)(st >> 16); }
        k[7] &= 0x3fffffffu;
        const G2Affine q = g2_mul(gen, k, 8);
        if (q.inf || !g2_in_subgroup(q) || !g2_killed_by_r(q)) { printf("multiple %d of the generator fails\n", t); bad++; }
        on_subgroup++;
    }
    for (uint32_t c = 0; off_subgroup < 6 && c < 200; c++) {  // points of E'(Fp2) over x = c + u
        Fp xc = zero<FpParams>();
        xc.v[0] = c;
        G2Affine q;
        if (!g2_from_x(q, Fp2{to_mont(xc), one<FpParams>()})) continue;
        const bool fast = g2_in_subgroup(q), slow = g2_killed_by_r(q);
        if (fast || slow) { printf("x = %u + u: psi test %d, [r]Q test %d (a random curve point is not in the subgroup)\n", c, fast, slow); bad++; }
        off_subgroup++;
    }
    if (off_subgroup < 6) { printf("found only %d curve points\n", off_subgroup); bad++; }
    if (argc > 2) {
        FILE* f = fopen(argv[2], "rb");
        std::vector<uint8_t> b;
        if (f) {
            uint8_t buf[4096];
            size_t n;
            while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
            fclose(f);
        }
        if (!f || b.empty() || b.size() % 96) { printf("cannot read %s as 96-byte points\n", argv[2]); bad++; }
        for (size_t i = 0; f && i + 96 <= b.size() && b.size() % 96 == 0; i += 96) {
            G2Affine q;
            if (!g2_decompress(q, b.data() + i)) { printf("constructed point %zu does not decode to a curve point\n", i / 96); bad++; continue; }
            const bool fast = g2_in_subgroup(q), slow = g2_killed_by_r(q);
            if (fast || slow) { printf("constructed point %zu: psi test %d, [r]Q test %d\n", i / 96, fast, slow); bad++; }
            else off_subgroup++;
        }
    }
    {
        const G2Affine inf = {Fp2{zero<FpParams>(), zero<FpParams>()}, Fp2{zero<FpParams>(), zero<FpParams>()}, true};
        uint8_t enc[96] = {0xc0};
        G2Affine dec;
        if (!g2_decompress(dec, enc) || !dec.inf || !g2_in_subgroup(dec) || !g2_in_subgroup(inf) || !g2_killed_by_r(inf)) { printf("infinity is not handled as the identity\n"); bad++; }
    }
    {   // sum_j k_j Q_j with shared doublings against the single multiples added one by one (through the pairing-free equality)
        uint32_t k[5][4];
        for (auto& row : k) for (auto& w : row) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; w = (uint32_t)(st >> 16); }
        const G2Affine sum = g2_lincomb128(pts.data() + 1, k, 5);
        G2Jac acc = g2j_inf();
        for (int j = 0; j < 5; j++) acc = g2j_add(acc, g2j_from(g2_mul(pts[1 + j], k[j], 4)));
        if (!g2_eq(sum, g2j_to_affine(acc)) || sum.inf) { printf("g2_lincomb128 differs from the sum of its terms\n"); bad++; }
        if (!g2_in_subgroup(sum)) { printf("a sum of subgroup points fails the test\n"); bad++; }
    }
    printf("g2 subgroup test: %d on the subgroup, %d off it, %d mismatches\n", on_subgroup, off_subgroup, bad);
    return bad ? 1 : 0;
}
