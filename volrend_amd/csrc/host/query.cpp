// query.cpp -- volrend::query_points / query_grid over vr_query_points / vr_query_grid.
#include "volrend/query.hpp"

#include "volrend/internal/check.hpp"

namespace volrend {

void query_points(const N3Tree& tree, int64_t n, const float* xyz_dev, const float* dirs_dev,
                  const QueryOut& out, void* stream, QuerySpace space) {
    internal::vr_check(vr_query_points(tree.device, n, xyz_dev, dirs_dev, static_cast<int>(space), &out, stream),
                       "vr_query_points");
}

void query_grid(const N3Tree& tree, const std::array<float, 3>& lo, const std::array<float, 3>& hi,
                const std::array<int32_t, 3>& res, const float* dir, const QueryOut& out, void* stream,
                QuerySpace space) {
    internal::vr_check(vr_query_grid(tree.device, lo.data(), hi.data(), res.data(), dir, static_cast<int>(space),
                                     &out, stream),
                       "vr_query_grid");
}

}  // namespace volrend
