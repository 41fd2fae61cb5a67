// CPU run of the pieces of csrc/verify_host.hpp that eth_kzg_amd_verify_partial_data_columns adds: validate_partial_columns_call,
// validate_partial_column (the stray-bit rule) and partial_column_entries, PartialColumns (made from a pointer list and from the flat
// array), vm_kept_partial_columns with the parts, chunks and copy runs over the unequal columns that go on, partial_column_view (a
// column's own unique list, re-ranked rows and pairs, against dedup_commitments of the EXPANDED problem), and the per-column transcript
// digests and ROOTs taken the way a pass takes them.  Reads a case file, one command per line, and prints one line per command;
// tests/test_partial_columns_host.py writes the cases and compares with values it computes from tests/partial_columns.py and hashlib.
//   call FLAGS NB NC NULLS   -> call <validate_partial_columns_call>   (NULLS: bits commitments, indices, present, cells, proofs, verified)
//   plan NB NC MIN_PROBLEMS MIN_CELLS MAX_PARTS CHUNK  then per column: INDEX w_0 .. w_W-1 (hex words)
//        -> plan status,.. | m,.. | start,.. | keep,.. | parts,.. | chunks,.. | runs src:len:dst,.. | <1: list form == flat form>
//   view NB c_0 .. c_NB-1 M b_0 .. b_M-1
//        -> view uniq,.. | own rows | pass rows | pair_u | <1: uniq and rows equal dedup_commitments of the expanded problem, P <= M>
//   digests NB NC then per column INDEX w_0 .. w_W-1, then COMMITMENTS CELLS PROOFS (the packed device arrays)
//        -> digests D_0:ROOT_0,..   (per accepted column: the reference transcript's digest and the leaf-hashed ROOT; "-" for a refused one)
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
    if (want) in >> t;
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
template <class V>
static void print_list(const V& v, const char* end) {
    for (size_t i = 0; i < v.size(); i++) printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
    printf("%s", end);
}
// the columns of a command: per column its index and W words -> (indices, flat words)
static void read_columns(std::istream& in, uint64_t nb, uint64_t nc, std::vector<uint64_t>& index, std::vector<uint64_t>& flat) {
    const uint64_t W = partial_words(nb);
    index.resize(nc);
    flat.assign(nc * W, 0);
    for (uint64_t j = 0; j < nc; j++) {
        in >> std::dec >> index[j];
        for (uint64_t w = 0; w < W; w++) in >> std::hex >> flat[j * W + w];
    }
    in >> std::dec;
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
            printf("call %d\n", validate_partial_columns_call(flags, 1u, nb, nc, nulls & 1, nulls & 2, nulls & 4, nulls & 8, nulls & 16, nulls & 32));
        } else if (cmd == "plan") {
            uint64_t nb, nc, min_cells, chunk;
            int min_problems, max_parts;
            in >> nb >> nc >> min_problems >> min_cells >> max_parts >> chunk;
            std::vector<uint64_t> index, flat;
            const bool unread = nb > INPUT_MAX_CELLS;  // nothing of the bitmaps is read: the case carries none
            if (unread) { index.resize(nc); for (uint64_t& x : index) in >> x; }
            else read_columns(in, nb, nc, index, flat);
            const uint64_t W = partial_words(nb);
            // the list form reads exactly W words per column: every column's words in an allocation of their own
            std::vector<std::vector<uint64_t>> own(nc);
            std::vector<const uint64_t*> list(nc, nullptr);
            for (uint64_t j = 0; j < nc && !unread; j++) { own[j].assign(flat.begin() + j * W, flat.begin() + (j + 1) * W); list[j] = own[j].data(); }
            PartialColumns a, b;
            a.from_list(nb, nc, index.data(), unread ? nullptr : list.data());
            std::vector<uint64_t> exact(flat);  // (a copy of exactly nc W words)
            b.from_flat(nb, nc, index.data(), unread ? nullptr : exact.data());
            const bool same = a.status == b.status && a.count == b.count && a.start == b.start && a.blob_start == b.blob_start && a.blob == b.blob;
            const std::vector<uint64_t> keep = vm_kept_partial_columns(a, 0, nc);
            const int K = (int)keep.size();
            auto cells_of = [&](int k) { return a.count[keep[(size_t)k]]; };
            printf("plan ");
            print_list(a.status, " | ");
            print_list(a.count, " | ");
            print_list(a.start, " | ");
            print_list(keep, " | ");
            print_list(vm_call_parts(K, cells_of, min_problems, min_cells, max_parts), " | ");
            std::vector<int> ends{0};
            while (ends.back() < K) ends.push_back(vm_chunk_end(K, ends.back(), cells_of, chunk));
            print_list(ends, " | ");
            const std::vector<CopyRun> runs = vm_copy_runs(K, [&](int k) { return a.start[keep[(size_t)k]]; }, cells_of, [&](int k) { return cells_of(k) != 0; });
            for (size_t r = 0; r < runs.size(); r++)
                printf("%s%llu:%llu:%llu", r ? "," : "", (unsigned long long)runs[r].src, (unsigned long long)runs[r].len, (unsigned long long)runs[r].dst);
            printf(" | %d\n", same ? 1 : 0);
        } else if (cmd == "view") {
            size_t nb, m;
            in >> nb;
            std::vector<Bytes> comm(nb);
            std::vector<const uint8_t*> list(nb);
            for (size_t i = 0; i < nb; i++) { comm[i] = next_bytes(in, 48); list[i] = comm[i].data(); }
            in >> m;
            std::vector<uint32_t> blobs(m);
            for (uint32_t& x : blobs) in >> x;
            ColumnCommitments cc;
            cc.from_list(nb, list.data());
            PartialColumnView v;
            partial_column_view(cc, blobs.data(), m, v);
            // the expanded problem, de-duplicated alone
            std::vector<const uint8_t*> exp(m), eu;
            std::vector<int> er;
            for (size_t k = 0; k < m; k++) exp[k] = list[blobs[k]];
            dedup_commitments(m, exp.data(), eu, er);
            bool same = er == v.row && eu.size() == v.uniq.size() && v.pair_u.size() == v.uniq.size() && v.pair_u.size() <= m;
            for (size_t j = 0; same && j < eu.size(); j++) same = memcmp(eu[j], v.uniq[j], 48) == 0 && v.uniq[j] == cc.uniq[(size_t)v.pair_u[j]];
            for (size_t k = 0; same && k < m; k++) same = v.pass_row[k] == cc.row[blobs[k]] && v.pair_u[(size_t)v.row[k]] == v.pass_row[k];
            printf("view ");
            for (size_t j = 0; j < v.uniq.size(); j++) printf("%s%s", j ? "," : "", hex(v.uniq[j], 48).c_str());
            printf(" | ");
            print_list(v.row, " | ");
            print_list(v.pass_row, " | ");
            print_list(v.pair_u, " | ");
            printf("%d\n", same ? 1 : 0);
        } else if (cmd == "digests") {
            uint64_t nb, nc;
            in >> nb >> nc;
            std::vector<uint64_t> index, flat;
            read_columns(in, nb, nc, index, flat);
            PartialColumns pc;
            pc.from_flat(nb, nc, index.data(), flat.data());
            const uint64_t N = pc.start[nc];
            const Bytes comm = next_bytes(in, nb * 48), cells = next_bytes(in, N * BYTES_PER_CELL), proofs = next_bytes(in, N * 48);
            ColumnCommitments cc;
            cc.own = comm;
            cc.from_own(nb);
            printf("digests ");
            for (uint64_t j = 0; j < nc; j++) {  // as a pass takes them: the transcript over the column's own view, the leaves over the pass-wide rows
                if (pc.status[j] != INPUT_VALID) { printf("%s-", j ? "," : ""); continue; }
                const uint64_t m = pc.count[j];
                const uint8_t *cj = cells.data() + pc.start[j] * BYTES_PER_CELL, *pj = proofs.data() + pc.start[j] * 48;
                PartialColumnView v;
                partial_column_view(cc, pc.blob.data() + pc.blob_start[j], m, v);
                CellBatchTranscript t((int)v.uniq.size(), (int)m, v.uniq.data());
                Bytes leaves(m * 32 + 1);
                for (uint64_t k = 0; k < m; k++) {
                    t.absorb(v.row[k], index[j], cj + k * BYTES_PER_CELL, pj + k * 48);
                    CellLeafTranscript::leaf(k, index[j], cc.uniq[(size_t)v.pass_row[k]], pj + k * 48, cj + k * BYTES_PER_CELL, leaves.data() + 32 * k);
                }
                t.finish();
                CellLeafTranscript root;
                root.root(m, leaves.data());
                printf("%s%s:%s", j ? "," : "", hex(t.digest(), 32).c_str(), hex(root.digest(), 32).c_str());
            }
            printf("\n");
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
        if (!in) { fprintf(stderr, "a short line: %s\n", line.substr(0, 60).c_str()); return 2; }
    }
    return 0;
}
