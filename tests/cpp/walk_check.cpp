// walk_check -- drives volrend_amd/csrc/vr_tree_walk.cpp for tests/test_tree_walk.py.  Plain host
// build: no HIP, no library.
//   walk_check walk <child.bin> <cap> <N3> <G0> <BL>   child.bin: cap * N3 int32
//       -> "depth D" / "level ..." / "perm ..." / "roots ...", or "why <text>" for a bad tree
//   walk_check plan <N> <max_depth> <capacity> <top_levels> <brick_levels> <n_roots>   -> "G0 BL"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vr_tree_walk.h"

template <class T>
static void print_row(const char* name, const std::vector<T>& v) {
    printf("%s", name);
    for (const T& x : v) printf(" %lld", (long long)x);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc == 8 && !strcmp(argv[1], "plan")) {
        const uint64_t n_roots = strtoull(argv[7], nullptr, 10);
        const LookupPlan p = plan_lookup(atoi(argv[2]), atoi(argv[3]), atoll(argv[4]), atoi(argv[5]), atoi(argv[6]),
                                         [n_roots](int) { return n_roots; });
        printf("%d %d\n", p.G0, p.BL);
        return 0;
    }
    if (argc != 7 || strcmp(argv[1], "walk")) return 2;
    const int64_t cap = atoll(argv[3]);
    const int N3 = atoi(argv[4]), G0 = atoi(argv[5]), BL = atoi(argv[6]);
    std::vector<int32_t> child((size_t)(cap > 0 ? cap : 0) * N3);
    FILE* f = fopen(argv[2], "rb");
    if (!f || fread(child.data(), sizeof(int32_t), child.size(), f) != child.size()) return 3;
    fclose(f);
    char why[256] = "";
    std::vector<uint8_t> level;
    const int depth = validate_topology(child.data(), cap, N3, level, why, sizeof(why));
    if (depth < 0) {
        printf("why %s\n", why);
        return 0;
    }
    std::vector<int32_t> roots;
    const std::vector<int32_t> perm = node_permutation(child.data(), cap, N3, G0, BL, level, roots);
    printf("depth %d\n", depth);
    print_row("level", level);
    print_row("perm", perm);
    print_row("roots", roots);
    return 0;
}
