// volrend::accumulate_weights -- per leaf slot, the largest compositing weight any sample in it received
// from the rays of a set of views, and the number of hit samples in it, over the HIP C ABI
// (vr_accumulate_weights, include/volrend_hip.h).  What PlenOctree extraction and pruning threshold on
// (svox: accumulate_weights); the reference renderer has no counterpart.
// Asynchronous like launch_renderer: returns after enqueueing on `stream` (a hipStream_t passed as void*);
// throws std::runtime_error where the C call refuses its arguments.
#pragma once
#include <cstdint>
#include <vector>

#include "volrend/renderer_kernel.hpp"

namespace volrend {

// Device pointers (nullptr = not wanted, at least one wanted), both [capacity * N^3] and indexed like the
// file's child / data arrays: node * N^3 + child slot in the FILE's node numbering.
//   max_weight: max over the hit samples with weight > 0 of weight = light_intensity * (1 - att);
//   hits      : hit samples (sigma > sigma_thresh) in the slot, modulo 2^32.
// The call accumulates INTO both: zero them once, then any split of the poses into calls, streams or
// devices (merged with an element-wise max / sum) gives the same bits.  max_weight must hold non-negative,
// non-NaN floats on entry.
using LeafWeights = VrLeafWeights;

// transforms[i]: the 12-float column-major 4x3 c2w of pose i, every pose with cam's size and intrinsics;
// one launch per <= VR_MAX_BATCH poses (no pose: only the tree's file-order table is put on the device).
// Of `options` only step_size, sigma_thresh, stop_thresh and render_bbox are read.  fp_mode: VR_FP_STRICT
// or VR_FP_FMA.
void accumulate_weights(const N3Tree& tree, const Camera& cam, const std::vector<const float*>& transforms,
                        const RenderOptions& options, const LeafWeights& out, void* stream,
                        int fp_mode = VR_FP_STRICT);

}  // namespace volrend
