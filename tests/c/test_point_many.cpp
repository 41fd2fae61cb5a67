// CPU run of the host statement of eth_kzg_amd_verify_kzg_proof_many in csrc/verify_host.hpp: PointProofTranscript (leaf, seed), the
// weights fold_weight gives under that seed, point_pass_end and point_item_status.  Reads a case file, one command per line, and prints
// one line per command; tests/test_point_many_host.py writes the cases and compares with values it computes from hashlib and Python
// integers (tests/point_many.py).
//   leaf C Z Y P              -> leaf <LEAF>                         (hex: 48, 32, 32, 48 bytes)
//   seed N LEAVES             -> seed <SEED>                         (LEAVES: N * 32 bytes in hex, or - for none)
//   weights SEED N            -> weights rho_0,..,rho_N-1            (each as 32 hex digits of the integer)
//   bounds N P                -> bounds s_0,s_1,..,N                 (the first item of every pass of a call of N items cut at P, then N)
//   status CBAD PBAD Z Y      -> status <point_item_status>
#include "verify_host.hpp"
#include "sha256.cpp"

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
using namespace kzg;

typedef std::vector<uint8_t> Bytes;

static int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
static Bytes next_bytes(std::istream& in, size_t want) {
    std::string t;
    in >> t;
    if (want == 0 && t == "-") return Bytes();
    if (t.size() != 2 * want) { fprintf(stderr, "a byte string of %zu hex digits where %zu bytes are expected\n", t.size(), want); exit(2); }
    Bytes b(want);  // exactly the bytes the functions may read: a read past them is the sanitizer's to find
    for (size_t i = 0; i < want; i++) {
        const int hi = nibble(t[2 * i]), lo = nibble(t[2 * i + 1]);
        if (hi < 0 || lo < 0) { fprintf(stderr, "not a hex string\n"); exit(2); }
        b[i] = (uint8_t)(hi * 16 + lo);
    }
    return b;
}
static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    std::ifstream file(argv[1]);
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "leaf") {
            const Bytes c = next_bytes(in, 48), z = next_bytes(in, 32), y = next_bytes(in, 32), p = next_bytes(in, 48);
            uint8_t out[32];
            PointProofTranscript::leaf(c.data(), z.data(), y.data(), p.data(), out);
            printf("leaf %s\n", hex(out, 32).c_str());
        } else if (cmd == "seed") {
            uint64_t n;
            in >> n;
            Bytes leaves = next_bytes(in, (size_t)n * 32);
            leaves.reserve(1);
            uint8_t out[32];
            PointProofTranscript::seed(n, leaves.data(), out);
            printf("seed %s\n", hex(out, 32).c_str());
        } else if (cmd == "weights") {
            const Bytes seed = next_bytes(in, 32);
            uint64_t n;
            in >> n;
            printf("weights ");
            for (uint64_t i = 0; i < n; i++) {
                uint32_t w[4];
                fold_weight(seed.data(), i, w);
                printf("%s%08x%08x%08x%08x", i ? "," : "", w[3], w[2], w[1], w[0]);
            }
            printf("\n");
        } else if (cmd == "bounds") {
            uint64_t n, pass;
            in >> n >> pass;
            printf("bounds ");
            for (uint64_t lo = 0; lo < n; lo = point_pass_end(n, lo, pass)) printf("%llu,", (unsigned long long)lo);
            printf("%llu\n", (unsigned long long)n);
        } else if (cmd == "status") {
            int cbad, pbad;
            in >> cbad >> pbad;
            const Bytes z = next_bytes(in, 32), y = next_bytes(in, 32);
            printf("status %d\n", point_item_status(cbad != 0, pbad != 0, z.data(), y.data()));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
