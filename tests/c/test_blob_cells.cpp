// CPU run of the host statement of eth_kzg_amd_verify_blob_cell_proofs_many in csrc/verify_host.hpp, the blob source of the cell
// many-verification: the status of an item (blob_cells_item_status), what the call refuses as a whole (validate_blob_cells_call), where
// an item's blob and extension lie in a pass's cells (blob_cells_slice), and the pass's plans over items of 128 cells (vm_call_parts,
// vm_chunk_end with blob_cells_of).  Reads a case file, one command per line, and prints one line per command;
// tests/test_blob_cells_host.py writes the cases and compares with values it works out itself (tests/blob_cells.py).
//   merge BLOBBAD POINTBAD                  -> merge <status>
//   call N BLOBS COMMITMENTS PROOFS VERIFIED -> call <0 valid | 3 invalid>      (1 = that array is NULL)
//   slice I                                 -> slice <blob_at> <ext_at>
//   parts MIN_PROBLEMS MIN_CELLS MAX_PARTS N -> parts cut_0,cut_1,..
//   chunks CHUNK_CELLS N                    -> chunks 0,end_0,end_1,..
//   limits                                  -> limits <BLOB_CELLS_MAX_ITEMS> <cells per item>
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
        if (cmd == "merge") {
            int blob_bad, point_bad;
            in >> blob_bad >> point_bad;
            printf("merge %d\n", blob_cells_item_status(blob_bad != 0, point_bad != 0));
        } else if (cmd == "call") {
            uint64_t n;
            int b, c, p, v;
            in >> n >> b >> c >> p >> v;
            printf("call %d\n", validate_blob_cells_call(n, b != 0, c != 0, p != 0, v != 0));
        } else if (cmd == "slice") {
            uint64_t i;
            in >> i;
            const BlobCellsSlice s = blob_cells_slice((size_t)i);
            printf("slice %llu %llu\n", (unsigned long long)s.blob_at, (unsigned long long)s.ext_at);
        } else if (cmd == "parts") {
            int min_problems, max_parts, n;
            uint64_t min_cells;
            in >> min_problems >> min_cells >> max_parts >> n;
            print_list("parts", vm_call_parts(n, [](int b) { return blob_cells_of((uint64_t)b); }, min_problems, min_cells, max_parts));
        } else if (cmd == "chunks") {
            uint64_t chunk;
            int n;
            in >> chunk >> n;
            std::vector<int> ends{0};
            while (ends.back() < n) ends.push_back(vm_chunk_end(n, ends.back(), [](int b) { return blob_cells_of((uint64_t)b); }, chunk));
            print_list("chunks", ends);
        } else if (cmd == "limits") {
            printf("limits %llu %llu\n", (unsigned long long)BLOB_CELLS_MAX_ITEMS, (unsigned long long)blob_cells_of(0));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
