// CPU run of the host statement of eth_kzg_amd_verify_blob_kzg_proof_many in csrc/verify_host.hpp: the status of an item (blob_item_status),
// which items are live and what the call hands out (blob_item_live, blob_item_verified), the challenge z of an item as the leaf takes it
// (blob_challenge, 32 canonical bytes), and the passes of a call at the blob source's pass size.  Reads a case file, one command per
// line, and prints one line per command; tests/test_blob_many_host.py writes the cases and compares with values it computes itself.
//   merge BLOBBAD CST PST PASSED -> merge <status> <live> <verified>     (CST / PST: what the decoding left for commitment / proof)
//   challenge SEED COMMITMENT    -> challenge <z>                        (the blob: 4096 x SHA-256(SEED | be64(i)) with the top byte cleared)
//   bounds N                     -> bounds s_0,s_1,..,N                  (cut at BLOB_MANY_PASS)
//   limits                       -> limits <BLOB_MANY_MAX_ITEMS> <BLOB_MANY_PASS>
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
        if (cmd == "merge") {
            int blob_bad, cst, pst, passed;
            in >> blob_bad >> cst >> pst >> passed;
            const int st = blob_item_status(blob_bad != 0, cst, pst);
            printf("merge %d %d %d\n", st, blob_item_live(st) ? 1 : 0, blob_item_verified(st, passed != 0) ? 1 : 0);
        } else if (cmd == "challenge") {
            const Bytes seed = next_bytes(in, 8), commitment = next_bytes(in, 48);
            Bytes blob((size_t)BYTES_PER_BLOB);
            for (int i = 0; i < N_BLOB; i++) {
                uint8_t ix[8];
                be64((uint64_t)i, ix);
                Sha256 sh;
                sh.update(seed.data(), 8);
                sh.update(ix, 8);
                sh.finish(blob.data() + 32 * (size_t)i);
                blob[32 * (size_t)i] = 0;
            }
            uint8_t z[32];
            fr_to_be(z, from_mont(blob_challenge(blob.data(), commitment.data())));
            printf("challenge %s\n", hex(z, 32).c_str());
        } else if (cmd == "bounds") {
            uint64_t n;
            in >> n;
            printf("bounds ");
            for (uint64_t lo = 0; lo < n; lo = point_pass_end(n, lo, (uint64_t)BLOB_MANY_PASS)) printf("%llu,", (unsigned long long)lo);
            printf("%llu\n", (unsigned long long)n);
        } else if (cmd == "limits") {
            printf("limits %llu %d\n", (unsigned long long)BLOB_MANY_MAX_ITEMS, BLOB_MANY_PASS);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
