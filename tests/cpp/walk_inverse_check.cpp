// walk_inverse_check -- drives node_permutation + inverse_permutation of volrend_amd/csrc/vr_tree_walk.cpp
// for tests/test_weights_file_order.py.  Plain host build: no HIP, no library.
//   walk_inverse_check <child.bin> <cap> <N3> <G0> <BL>   child.bin: cap * N3 int32
//       -> "perm ..." (file node -> device node) / "file_node ..." (device node -> file node)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vr_tree_walk.h"

static void print_row(const char* name, const std::vector<int32_t>& v) {
    printf("%s", name);
    for (int32_t x : v) printf(" %d", x);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const int64_t cap = atoll(argv[2]);
    const int N3 = atoi(argv[3]), G0 = atoi(argv[4]), BL = atoi(argv[5]);
    if (cap <= 0) return 2;
    std::vector<int32_t> child((size_t)cap * N3);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(child.data(), sizeof(int32_t), child.size(), f) != child.size()) return 3;
    fclose(f);
    char why[256] = "";
    std::vector<uint8_t> level;
    if (validate_topology(child.data(), cap, N3, level, why, sizeof(why)) < 0) return 4;
    std::vector<int32_t> roots;
    const std::vector<int32_t> perm = node_permutation(child.data(), cap, N3, G0, BL, level, roots);
    print_row("perm", perm);
    print_row("file_node", inverse_permutation(perm));
    return 0;
}
