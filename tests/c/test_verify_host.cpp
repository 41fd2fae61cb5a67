// CPU run of csrc/verify_host.hpp: the validations, the de-duplication, the scalar codecs and the Fiat-Shamir transcripts that
// verify.hip, verify_many.hip and eip4844.hip share.  Reads a case file (one command per line, byte strings in hex) and prints one
// line of results per command; tests/test_host_units.py writes the cases and compares with hashlib and Python integers.
//   dedup N c_0 .. c_N-1                          -> dedup m row_0,..,row_N-1 uniq_0..uniq_m-1 (concatenated)
//   cell N (c_k index_k cell_k proof_k) x N       -> cell challenge digest
//   validate nc ni ncells np K index_0 .. index_K-1 -> validate code
//   reduce digest                                 -> reduce value
//   canonical bytes32                             -> canonical accepted value-or-dash
//   blob blob commitment                          -> blob challenge
//   blobbatch N (c_i z_i y_i proof_i) x N         -> blobbatch weight
//   fold digests i                                -> fold seed w0 w1 w2 w3
//   brp7                                          -> brp7 v_0,..,v_127
// Scalars are printed canonical, big-endian.
#include "verify_host.hpp"
#include "sha256.cpp"

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
using namespace kzg;

typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const std::string& s) {
    Bytes b(s.size() / 2);
    for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::stoi(s.substr(2 * i, 2), nullptr, 16);
    return b;
}
static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s;
}
static std::string fr_hex(const Fr& mont) {
    uint8_t b[32];
    fr_to_be(b, from_mont(mont));
    return hex(b, 32);
}
static Bytes next_bytes(std::istream& in, size_t want) {
    std::string t;
    in >> t;
    Bytes b = unhex(t);
    if (b.size() != want) { fprintf(stderr, "a byte string of %zu bytes where %zu are expected\n", b.size(), want); exit(2); }
    return b;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    std::ifstream file(argv[1]);
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "dedup" || cmd == "cell") {
            size_t n;
            in >> n;
            std::vector<Bytes> c(n), cells(n), proofs(n);
            std::vector<uint64_t> index(n);
            for (size_t k = 0; k < n; k++) {
                c[k] = next_bytes(in, 48);
                if (cmd == "cell") { in >> index[k]; cells[k] = next_bytes(in, BYTES_PER_CELL); proofs[k] = next_bytes(in, 48); }
            }
            std::vector<const uint8_t*> cp(n), uniq;
            std::vector<int> row;
            for (size_t k = 0; k < n; k++) cp[k] = c[k].data();
            dedup_commitments(n, cp.data(), uniq, row);
            if (cmd == "dedup") {
                printf("dedup %zu ", uniq.size());
                for (size_t k = 0; k < n; k++) printf("%s%d", k ? "," : "", row[k]);
                printf(" ");
                for (const uint8_t* u : uniq) printf("%s", hex(u, 48).c_str());
                printf("\n");
            } else {
                CellBatchTranscript t((int)uniq.size(), (int)n, uniq.data());
                for (size_t k = 0; k < n; k++) t.absorb(row[k], index[k], cells[k].data(), proofs[k].data());
                const Fr r = t.finish();
                printf("cell %s %s\n", fr_hex(r).c_str(), hex(t.digest(), 32).c_str());
            }
        } else if (cmd == "validate") {
            uint64_t nc, ni, ncells, np;
            size_t k;
            in >> nc >> ni >> ncells >> np >> k;
            std::vector<uint64_t> index(k);
            for (auto& v : index) in >> v;
            printf("validate %d\n", validate_cell_batch(nc, ni, ncells, np, index.data()));
        } else if (cmd == "reduce") {
            printf("reduce %s\n", fr_hex(fr_from_digest(next_bytes(in, 32).data())).c_str());
        } else if (cmd == "canonical") {
            Fr x;
            const bool ok = fr_from_be_canonical(x, next_bytes(in, 32).data());
            printf("canonical %d %s\n", (int)ok, ok ? fr_hex(x).c_str() : "-");
        } else if (cmd == "blob") {
            const Bytes blob = next_bytes(in, BYTES_PER_BLOB), c = next_bytes(in, 48);
            printf("blob %s\n", fr_hex(blob_challenge(blob.data(), c.data())).c_str());
        } else if (cmd == "blobbatch") {
            size_t n;
            in >> n;
            std::vector<Bytes> c(n), proofs(n);
            std::vector<Fr> z(n), y(n);
            std::vector<const uint8_t*> cp(n), pp(n);
            for (size_t i = 0; i < n; i++) {
                c[i] = next_bytes(in, 48);
                const Bytes zb = next_bytes(in, 32), yb = next_bytes(in, 32);
                proofs[i] = next_bytes(in, 48);
                if (!fr_from_be_canonical(z[i], zb.data()) || !fr_from_be_canonical(y[i], yb.data())) { fprintf(stderr, "z, y must be canonical\n"); return 2; }
                y[i] = from_mont(y[i]);  // the evaluations come from the GPU as canonical words, the points in Montgomery form
                cp[i] = c[i].data();
                pp[i] = proofs[i].data();
            }
            printf("blobbatch %s\n", fr_hex(blob_batch_weight((int)n, cp.data(), z.data(), y.data(), pp.data())).c_str());
        } else if (cmd == "fold") {
            std::string d;
            uint64_t i;
            in >> d >> i;
            const Bytes digests = unhex(d);
            uint8_t seed[32];
            uint32_t w[4];
            fold_seed(digests.data(), digests.size(), seed);
            fold_weight(seed, i, w);
            printf("fold %s %08x %08x %08x %08x\n", hex(seed, 32).c_str(), w[0], w[1], w[2], w[3]);
        } else if (cmd == "brp7") {
            printf("brp7 ");
            for (int v = 0; v < N_CELLS; v++) printf("%s%d", v ? "," : "", brp7(v));
            printf("\n");
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
