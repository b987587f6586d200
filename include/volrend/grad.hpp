// volrend::render_backward -- the derivative of a rendered batch with respect to the tree's values, over
// the HIP C ABI (vr_render_backward, include/volrend_hip.h, which has the formulas).  The step that follows
// pruning when a PlenOctree is optimised against its training images; the reference renderer has no
// counterpart.
// Asynchronous like launch_renderer: returns after enqueueing on `stream` (a hipStream_t passed as void*);
// throws std::runtime_error ("vr_render_backward: ...") where the C call refuses its arguments.
#pragma once
#include <cstdint>
#include <vector>

#include "volrend/renderer_kernel.hpp"

namespace volrend {

// transforms[i]: the 12-float column-major 4x3 c2w of pose i, every pose with cam's size and intrinsics; one
// launch per <= VR_MAX_BATCH poses (no pose: only the tree's file-order table is put on the device).
//   grad_accum  device, float32 [transforms.size()][height][width][4], tightly packed: dL / d of the four
//               numbers the pixel's accumulators receive (the background composite is the caller's);
//   grad_data   device, float32 [capacity * N^3 * data_dim], indexed like the file's data array; the call
//               ADDS into it (zero it once); elements no hit sample touches are not written.
// The sum uses float atomics: two runs may differ in the last bits.  The frame is marched as
// accumulate_weights marches it; render_depth, enable_probe, rot_dirs, a basis_minmax that leaves out a basis
// function of the tree and SG / ASG trees are refused.  fp_mode: VR_FP_STRICT or VR_FP_FMA.
void render_backward(const N3Tree& tree, const Camera& cam, const std::vector<const float*>& transforms,
                     const RenderOptions& options, const float* grad_accum, float* grad_data, void* stream,
                     int fp_mode = VR_FP_STRICT);

// The same, and the slots the call adds into are marked in `touched` (vr_render_backward_touched): device,
// ceil(capacity * N^3 / 32) words, one bit per child slot in grad_data's slot order (bit s & 31 of word s >> 5);
// ORed into, zeroed once by the caller.  The set of marked slots is bit-reproducible.  What tree_step (step.hpp)
// consumes.
void render_backward(const N3Tree& tree, const Camera& cam, const std::vector<const float*>& transforms,
                     const RenderOptions& options, const float* grad_accum, float* grad_data, uint32_t* touched,
                     void* stream, int fp_mode = VR_FP_STRICT);

}  // namespace volrend
