// volrend::query_points / query_grid -- bulk point queries on the uploaded tree, over the HIP C ABI
// (vr_query_points / vr_query_grid, include/volrend_hip.h): query_single_from_root
// (include/volrend/internal/n3tree_query.hpp:13-48) for many points in one launch, the record of
// the leaf each point falls in, and the colour a sample there has along a direction.  The reference
// has this per point only (retrieve_cursor_lumisphere_kernel, src/cuda/volrend.cu:175-191).
// Asynchronous like launch_renderer: returns after enqueueing on `stream`; throws
// std::runtime_error where the C call refuses its arguments.
#pragma once
#include <array>
#include <cstdint>

#include "volrend/n3tree.hpp"

namespace volrend {

enum class QuerySpace : int {
    World = VR_SPACE_WORLD,  // tree coordinate = offset + scale * x
    Tree = VR_SPACE_TREE     // x is a tree coordinate already
};

// Device pointers of the wanted outputs (nullptr = not wanted, at least one wanted):
//   sigma [n], depth [n] (int32), local [n][3], coeffs [n][data_dim - 1], rgb [n][3].
// rgb needs directions; it is evaluated at the direction AS GIVEN (not normalised), in the strict
// floating-point model, and is not available for SG / ASG trees.
using QueryOut = VrQueryOut;

// xyz_dev [n][3], dirs_dev [n][3] or nullptr: device float32 on the tree's device.
void query_points(const N3Tree& tree, int64_t n, const float* xyz_dev, const float* dirs_dev,
                  const QueryOut& out, void* stream, QuerySpace space = QuerySpace::World);

// The cell centres of the box lo..hi cut into res[0] x res[1] x res[2] cells, generated on the
// device: cell (i, j, k) -> output index (i * res[1] + j) * res[2] + k.  dir: one direction for
// all cells, or nullptr.
void query_grid(const N3Tree& tree, const std::array<float, 3>& lo, const std::array<float, 3>& hi,
                const std::array<int32_t, 3>& res, const float* dir, const QueryOut& out, void* stream,
                QuerySpace space = QuerySpace::World);

}  // namespace volrend
