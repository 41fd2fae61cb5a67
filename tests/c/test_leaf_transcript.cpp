// CPU run of csrc/verify_host.hpp: CellLeafTranscript, the host's statement of the cell verifier's leaf-hashed challenge.  Reads a case
// file (one batch per line, byte strings in hex) and prints one line per batch; tests/test_leaf_transcript_host.py writes the cases and
// compares with tests/leaf_transcript.py (hashlib).
//   batch N (commitment_k index_k cell_k proof_k) x N   -> batch LEAF_0,..,LEAF_N-1 ROOT r
// r is printed canonical, big-endian.
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
    Bytes b(want);
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
        if (cmd != "batch") { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
        size_t n;
        in >> n;
        std::vector<uint8_t> leaves(n * 32);
        printf("batch ");
        for (size_t k = 0; k < n; k++) {
            const Bytes c = next_bytes(in, 48);
            uint64_t index;
            in >> index;
            const Bytes cell = next_bytes(in, BYTES_PER_CELL), proof = next_bytes(in, 48);
            CellLeafTranscript::leaf(k, index, c.data(), proof.data(), cell.data(), leaves.data() + 32 * k);
            printf("%s%s", k ? "," : "", hex(leaves.data() + 32 * k, 32).c_str());
        }
        CellLeafTranscript t;
        const Fr r = t.root(n, leaves.data());
        uint8_t rb[32];
        fr_to_be(rb, from_mont(r));
        printf(" %s %s\n", hex(t.digest(), 32).c_str(), hex(rb, 32).c_str());
    }
    return 0;
}
