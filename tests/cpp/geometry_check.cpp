// geometry_check -- volrend::tree_geometry / slot_points (include/volrend/geometry.hpp) on a real GPU.  Driven by
// tests/test_gpu_cpp_geometry.py, which computes the same digests from the numpy restatement of
// tests/geometry_util.py.
//
//   geometry_check <child.raw> <N> <capacity> <slots.raw> <n> <k> <mode> <seed>
// child.raw: capacity * N^3 int32; slots.raw: n int32.  Runs tree_geometry with every output, then slot_points on the
// node_depth / node_origin it wrote, on one stream, and prints one "name digest" line per output: digest = sum over
// the 32-bit words w_i of (w_i + 1) * ((2 i + 1) * K) mod 2^64, K = 0x9E3779B97F4A7C15.  Also checks that refused
// calls throw.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "volrend/geometry.hpp"

#define HIP_OK(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 4;                                                             \
        }                                                                         \
    } while (0)

static bool read_raw(const char* path, std::vector<int32_t>& v) {
    std::ifstream f(path, std::ios::binary);
    return (bool)f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(int32_t)));
}

static int print_digest(const char* name, const void* dev, size_t words) {
    std::vector<uint32_t> w(words);
    HIP_OK(hipMemcpy(w.data(), dev, words * 4, hipMemcpyDeviceToHost));
    uint64_t d = 0;
    for (size_t i = 0; i < words; ++i) d += ((uint64_t)w[i] + 1u) * ((2u * (uint64_t)i + 1u) * 0x9E3779B97F4A7C15ull);
    printf("%s %016llx\n", name, (unsigned long long)d);
    return 0;
}

int main(int argc, char* argv[]) {
    using namespace volrend;
    if (argc < 9) return 2;
    const int N = atoi(argv[2]), k = atoi(argv[6]), mode = atoi(argv[7]);
    const int64_t cap = atoll(argv[3]), n = atoll(argv[5]);
    const uint32_t seed = (uint32_t)strtoul(argv[8], nullptr, 10);
    const size_t slots_of_tree = (size_t)cap * N * N * N;
    std::vector<int32_t> child(slots_of_tree), slots((size_t)n);
    if (!read_raw(argv[1], child) || !read_raw(argv[4], slots)) return 5;
    try {
        hipStream_t stream;
        HIP_OK(hipStreamCreate(&stream));
        int32_t *child_dev, *slots_dev, *parent, *node_depth, *depth;
        uint32_t* origin;
        float *points, *side;
        HIP_OK(hipMalloc((void**)&child_dev, slots_of_tree * 4));
        HIP_OK(hipMalloc((void**)&slots_dev, (size_t)n * 4));
        HIP_OK(hipMalloc((void**)&parent, (size_t)cap * 4));
        HIP_OK(hipMalloc((void**)&node_depth, (size_t)cap * 4));
        HIP_OK(hipMalloc((void**)&origin, (size_t)cap * 12));
        HIP_OK(hipMalloc((void**)&points, (size_t)n * k * 12));
        HIP_OK(hipMalloc((void**)&depth, (size_t)n * 4));
        HIP_OK(hipMalloc((void**)&side, (size_t)n * 4));
        HIP_OK(hipMemcpy(child_dev, child.data(), slots_of_tree * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(slots_dev, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice));

        Geometry g;
        g.child = child_dev;
        g.N = N;
        g.capacity = cap;
        g.parent_slot = parent;
        g.node_depth = node_depth;
        g.node_origin = origin;
        SlotPoints p;
        p.slots = slots_dev;
        p.n = n;
        p.k = k;
        p.mode = static_cast<PointsMode>(mode);
        p.seed = seed;
        p.points = points;
        p.depth = depth;
        p.side = side;
        tree_geometry(g, stream);
        slot_points(g, p, stream);  // (ordered behind the geometry by the stream)
        HIP_OK(hipStreamSynchronize(stream));
        if (print_digest("parent_slot", parent, (size_t)cap) || print_digest("node_depth", node_depth, (size_t)cap) ||
            print_digest("node_origin", origin, (size_t)cap * 3) || print_digest("points", points, (size_t)n * k * 3) ||
            print_digest("depth", depth, (size_t)n) || print_digest("side", side, (size_t)n))
            return 4;

        int threw = 0;
        try {
            Geometry bad = g;
            bad.parent_slot = bad.node_depth = nullptr;
            bad.node_origin = nullptr;
            tree_geometry(bad, stream);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_tree_geometry") != std::string::npos;
        }
        try {
            SlotPoints bad = p;
            bad.k = 65;
            slot_points(g, bad, stream);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_slot_points") != std::string::npos &&
                     std::string(e.what()).find("k=") != std::string::npos;
        }
        printf("throws %d\n", threw);
        for (void* q : {(void*)child_dev, (void*)slots_dev, (void*)parent, (void*)node_depth, (void*)origin, (void*)points,
                        (void*)depth, (void*)side})
            HIP_OK(hipFree(q));
        HIP_OK(hipStreamDestroy(stream));
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    return 0;
}
