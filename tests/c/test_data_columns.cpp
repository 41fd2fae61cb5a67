// CPU run of the pieces of csrc/verify_host.hpp that eth_kzg_amd_verify_data_columns adds: validate_data_columns_call,
// validate_data_column (against validate_cell_batch of the expanded problem), ColumnCommitments (the one de-duplication of a call,
// against dedup_commitments run per column), and the per-column transcript digests and ROOTs taken over that shared list.
// Reads a case file, one command per line, and prints one line per command; tests/test_data_columns_host.py writes the cases and
// compares with values it computes from hashlib (tests/data_columns.py, tests/verify_transcript.py, tests/leaf_transcript.py).
//   call FLAGS NB NC NULLS        -> call <validate_data_columns_call>   (NULLS: bits commitments, indices, cells, proofs, verified)
//   column NB INDEX               -> column <validate_data_column> <1: validate_cell_batch of the expanded problem says the same; NB <= 4096>
//   dedup NC N c_0 .. c_N-1       -> dedup M row_0,.. uniq_0,.. <1: the list form, the flat form and NC per-column runs agree>
//   digests NB NC i_0 .. i_NC-1 COMMITMENTS CELLS PROOFS
//                                 -> digests D_0:ROOT_0,..   (per column: the reference transcript's digest and the leaf-hashed ROOT)
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
        if (cmd == "call") {
            uint32_t flags;
            uint64_t nb, nc;
            unsigned nulls;
            in >> flags >> nb >> nc >> nulls;
            printf("call %d\n", validate_data_columns_call(flags, 1u, nb, nc, nulls & 1, nulls & 2, nulls & 4, nulls & 8, nulls & 16));
        } else if (cmd == "column") {
            uint64_t nb, index;
            in >> nb >> index;
            const int st = validate_data_column(nb, index);
            int same = 1;
            if (nb <= 4096) {  // the expanded problem: four equal lengths, nb copies of the index (exactly nb entries: none when nb is 0)
                std::vector<uint64_t> ix(nb, index);
                same = validate_cell_batch(nb, nb, nb, nb, nb ? ix.data() : nullptr) == st;
            } else if (nb > INPUT_MAX_CELLS) {
                same = validate_cell_batch(nb, nb, nb, nb, nullptr) == st;  // (refused before an index is read)
            }
            printf("column %d %d\n", st, same);
        } else if (cmd == "dedup") {
            size_t nc, n;
            in >> nc >> n;
            std::vector<Bytes> own(n);
            ColumnCommitments flat;
            for (size_t k = 0; k < n; k++) {
                own[k] = next_bytes(in, 48);
                flat.own.insert(flat.own.end(), own[k].begin(), own[k].end());
            }
            std::vector<const uint8_t*> list(n);
            for (size_t k = 0; k < n; k++) list[k] = own[k].data();
            ColumnCommitments shared;
            shared.from_list(n, list.data());
            flat.from_own(n);
            bool same = shared.row == flat.row && shared.uniq.size() == flat.uniq.size();
            for (size_t j = 0; same && j < flat.uniq.size(); j++) same = memcmp(shared.uniq[j], flat.uniq[j], 48) == 0;
            for (size_t c = 0; c < nc && same; c++) {  // what the expanded call does: every column de-duplicates its own copy of the list
                std::vector<Bytes> copy = own;
                std::vector<const uint8_t*> lc(n), uc;
                std::vector<int> rc;
                for (size_t k = 0; k < n; k++) lc[k] = copy[k].data();
                dedup_commitments(n, lc.data(), uc, rc);
                same = rc == shared.row && uc.size() == shared.uniq.size();
                for (size_t j = 0; same && j < uc.size(); j++) same = memcmp(uc[j], shared.uniq[j], 48) == 0;
            }
            printf("dedup %zu ", shared.uniq.size());
            for (size_t k = 0; k < n; k++) printf("%s%d", k ? "," : "", shared.row[k]);
            printf(" ");
            for (size_t j = 0; j < shared.uniq.size(); j++) printf("%s%s", j ? "," : "", hex(shared.uniq[j], 48).c_str());
            printf(" %d\n", same ? 1 : 0);
        } else if (cmd == "digests") {
            size_t nb, nc;
            in >> nb >> nc;
            std::vector<uint64_t> index(nc);
            for (uint64_t& x : index) in >> x;
            const Bytes comm = next_bytes(in, nb * 48), cells = next_bytes(in, nc * nb * BYTES_PER_CELL), proofs = next_bytes(in, nc * nb * 48);
            ColumnCommitments cc;
            cc.own = comm;
            cc.from_own(nb);
            printf("digests ");
            for (size_t j = 0; j < nc; j++) {  // as a pass takes them: every column over the call's one uniq / row pair
                const uint8_t *cj = cells.data() + j * nb * BYTES_PER_CELL, *pj = proofs.data() + j * nb * 48;
                CellBatchTranscript t((int)cc.uniq.size(), (int)nb, cc.uniq.data());
                Bytes leaves(nb * 32);
                for (size_t i = 0; i < nb; i++) {
                    t.absorb(cc.row[i], index[j], cj + i * BYTES_PER_CELL, pj + i * 48);
                    CellLeafTranscript::leaf(i, index[j], cc.uniq[(size_t)cc.row[i]], pj + i * 48, cj + i * BYTES_PER_CELL, leaves.data() + 32 * i);
                }
                t.finish();
                CellLeafTranscript root;
                root.root(nb, leaves.data());
                printf("%s%s:%s", j ? "," : "", hex(t.digest(), 32).c_str(), hex(root.digest(), 32).c_str());
            }
            printf("\n");
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
