// CPU run of the bookkeeping of the cell many-verification in csrc/verify_host.hpp: vm_call_parts, vm_chunk_end, vm_copy_runs,
// vm_kept_columns.  Reads a case file, one command per line, and prints one line per command; tests/test_vm_plan_host.py writes the
// cases and compares with what it works out from its own statement of each rule.
//   parts MIN_PROBLEMS MIN_CELLS MAX_PARTS B c_0 .. c_B-1   -> parts cut_0,cut_1,..        (the cut points, 0 first and B last)
//   chunks CHUNK_CELLS B n_0 .. n_B-1                       -> chunks 0,end_0,end_1,..     (vm_chunk_end from 0 until B is reached)
//   runs B src_0 len_0 takes_0 .. src_B-1 len_B-1 takes_B-1 -> runs src:len:dst,..
//   keep N_BLOBS N_COLUMNS i_0 .. i_N-1                     -> keep k_0,k_1,..
#include "verify_host.hpp"

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
using namespace kzg;

template <class V>
static void print_list(const char* what, const V& v) {
    printf("%s ", what);
    for (size_t i = 0; i < v.size(); i++) printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    std::ifstream file(argv[1]);
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "parts") {
            int min_problems, max_parts, B;
            uint64_t min_cells;
            in >> min_problems >> min_cells >> max_parts >> B;
            std::vector<uint64_t> cells(B);
            for (uint64_t& c : cells) in >> c;
            print_list("parts", vm_call_parts(B, [&](int b) { return cells[(size_t)b]; }, min_problems, min_cells, max_parts));
        } else if (cmd == "chunks") {
            uint64_t chunk;
            int B;
            in >> chunk >> B;
            std::vector<uint64_t> n(B);
            for (uint64_t& c : n) in >> c;
            std::vector<int> ends{0};
            while (ends.back() < B) {
                const int e = vm_chunk_end(B, ends.back(), [&](int b) { return n[(size_t)b]; }, chunk);
                if (e <= ends.back() || e > B) { fprintf(stderr, "a chunk that ends at %d after %d\n", e, ends.back()); return 1; }
                ends.push_back(e);
            }
            print_list("chunks", ends);
        } else if (cmd == "runs") {
            int B;
            in >> B;
            std::vector<uint64_t> src(B), len(B);
            std::vector<int> takes(B);
            for (int b = 0; b < B; b++) in >> src[b] >> len[b] >> takes[b];
            const std::vector<CopyRun> runs =
                vm_copy_runs(B, [&](int b) { return src[(size_t)b]; }, [&](int b) { return len[(size_t)b]; }, [&](int b) { return takes[(size_t)b] != 0; });
            printf("runs ");
            for (size_t r = 0; r < runs.size(); r++)
                printf("%s%llu:%llu:%llu", r ? "," : "", (unsigned long long)runs[r].src, (unsigned long long)runs[r].len, (unsigned long long)runs[r].dst);
            printf("\n");
        } else if (cmd == "keep") {
            uint64_t nb, nc;
            in >> nb >> nc;
            std::vector<uint64_t> index(nc);
            for (uint64_t& x : index) in >> x;
            print_list("keep", vm_kept_columns(nb, nc, index.data()));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
        if (!in) { fprintf(stderr, "a short line: %s\n", line.substr(0, 60).c_str()); return 2; }
    }
    return 0;
}
