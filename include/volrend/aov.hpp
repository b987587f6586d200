// volrend::launch_renderer_aov -- launch_renderer that also writes per-pixel float planes from the
// same march (vr_render_aov, include/volrend_hip.h): the depth sum D = sum of weight * t of
// trace_ray (rt_core.cuh:66-196) and the transmittance the ray left the loop with.
// Asynchronous like launch_renderer; failures throw as launch_renderer's do.
#pragma once
#include <cstdint>
#include <vector>

#include "volrend/renderer_kernel.hpp"

namespace volrend {

// The planes of ONE frame: device pointers, nullptr = not wanted (at least one of the two).
// Always addressed in frame position: plane + y * pitch + 4 * x.
struct AovPlanes {
    float* depth = nullptr;          // [height] rows of width floats
    float* transmittance = nullptr;
    int64_t pitch = 0;               // bytes per row of both planes; 0 = width * 4
};

// What the depth plane holds:
//   Tree : D, a distance along the normalised tree-space direction;
//   World: D * delta_scale, the length the attenuation uses (rt_core.cuh:119) -- for an NDC tree a
//          length in NDC space.
// The expected depth of what a ray hit is depth / (1 - transmittance); the library does not form it.
enum class DepthUnits : int { Tree = 0, World = 1 };

void launch_renderer_aov(const N3Tree& tree, const Camera& cam, const RenderOptions& options,
                         void* image_rgba8_dev, const float* depth_dev, const AovPlanes& aov,
                         DepthUnits depth_units, void* stream, bool offscreen = false);

// transforms[i] -> images[i], aovs[i]; one launch per <= VR_MAX_BATCH poses.
void launch_renderer_aov_batch(const N3Tree& tree, const Camera& cam,
                               const std::vector<const float*>& transforms, const RenderOptions& options,
                               const std::vector<void*>& images, const std::vector<AovPlanes>& aovs,
                               DepthUnits depth_units, void* stream, bool offscreen = true);

}  // namespace volrend
