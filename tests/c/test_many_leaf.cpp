// CPU run of the pieces of csrc/verify_host.hpp that the many-verification's flat device source and leaf-hashed challenges add:
// validate_cell_starts, dedup_commitments_flat (against dedup_commitments on a pointer list over the same bytes) and cell_leaf_root.
// Reads a case file, one command per line, and prints one line per command; tests/test_many_leaf_host.py writes the cases and compares
// with values it computes from hashlib (tests/many_leaf.py, tests/leaf_transcript.py).
//   starts NB v_0 .. v_NB         -> starts <validate_cell_starts>          (NB + 1 entries; none when NB is 0)
//   starts-null NB                -> starts <validate_cell_starts(NB, NULL)>
//   size N                        -> size <validate_cell_batch(N, N, N, N, no indices)>   (N = 0, or N above the bound: no index is read)
//   dedup N c_0 .. c_N-1          -> dedup M row_0,..,row_N-1 uniq_0,..,uniq_M-1 <1: the flat and the pointer-list form agree>
//   roots NB v_0 .. v_NB LEAVES   -> roots ROOT_0:r_0,..   (LEAVES: (v_NB - v_0) * 32 bytes in hex, or - for none; r canonical big-endian)
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
static std::vector<uint64_t> next_starts(std::istream& in, uint64_t nb) {
    std::vector<uint64_t> v(nb + 1);  // exactly the entries the functions may read: a read past them is the sanitizer's to find
    for (uint64_t& x : v) in >> x;
    return v;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    std::ifstream file(argv[1]);
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "starts") {
            uint64_t nb;
            in >> nb;
            if (nb == 0) { printf("starts %d\n", validate_cell_starts(0, nullptr)); continue; }
            const std::vector<uint64_t> v = next_starts(in, nb);
            printf("starts %d\n", validate_cell_starts(nb, v.data()));
        } else if (cmd == "starts-null") {
            uint64_t nb;
            in >> nb;
            printf("starts %d\n", validate_cell_starts(nb, nullptr));
        } else if (cmd == "size") {
            uint64_t n;
            in >> n;
            if (n != 0 && n <= INPUT_MAX_CELLS) { fprintf(stderr, "size: a count that reads no index\n"); return 2; }
            printf("size %d\n", validate_cell_batch(n, n, n, n, nullptr));
        } else if (cmd == "dedup") {
            size_t n;
            in >> n;
            Bytes flat;
            std::vector<Bytes> own(n);  // the pointer-list form over separate allocations
            for (size_t k = 0; k < n; k++) {
                own[k] = next_bytes(in, 48);
                flat.insert(flat.end(), own[k].begin(), own[k].end());
            }
            std::vector<const uint8_t*> list(n), uniq_list, uniq_flat;
            for (size_t k = 0; k < n; k++) list[k] = own[k].data();
            std::vector<int> row_list, row_flat;
            dedup_commitments(n, list.data(), uniq_list, row_list);
            dedup_commitments_flat(n, flat.data(), uniq_flat, row_flat);
            bool same = row_list == row_flat && uniq_list.size() == uniq_flat.size();
            for (size_t j = 0; same && j < uniq_flat.size(); j++) same = memcmp(uniq_list[j], uniq_flat[j], 48) == 0;
            for (const uint8_t* u : uniq_flat) same = same && u >= flat.data() && u + 48 <= flat.data() + flat.size() && (u - flat.data()) % 48 == 0;
            printf("dedup %zu ", uniq_flat.size());
            for (size_t k = 0; k < n; k++) printf("%s%d", k ? "," : "", row_flat[k]);
            printf(" ");
            for (size_t j = 0; j < uniq_flat.size(); j++) printf("%s%s", j ? "," : "", hex(uniq_flat[j], 48).c_str());
            printf(" %d\n", same ? 1 : 0);
        } else if (cmd == "roots") {
            uint64_t nb;
            in >> nb;
            const std::vector<uint64_t> v = next_starts(in, nb);
            Bytes leaves = next_bytes(in, (size_t)(v[nb] - v[0]) * 32);
            leaves.reserve(1);  // (a call of empty problems only: still an address, as the pass's slab is)
            printf("roots ");
            for (uint64_t b = 0; b < nb; b++) {
                uint8_t root[32], rb[32];
                const Fr r = cell_leaf_root(leaves.data(), v.data(), (size_t)b, root);
                fr_to_be(rb, from_mont(r));
                printf("%s%s:%s", b ? "," : "", hex(root, 32).c_str(), hex(rb, 32).c_str());
            }
            printf("\n");
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
