// volrend::render_rays / accumulate_weights_rays / render_backward_rays / fit_rays -- colour, leaf weights,
// gradients and the fused L2 loss + gradient along caller-supplied rays, over the HIP C ABI (vr_render_rays,
// vr_accumulate_weights_rays, vr_render_backward_rays, vr_fit_rays; include/volrend_hip.h has the semantics).  What an optimiser of a PlenOctree calls
// per step with rays drawn from all its training images; the reference renderer has no counterpart.
// Asynchronous like launch_renderer: each returns after enqueueing one launch on `stream` (a hipStream_t passed
// as void*); each throws std::runtime_error ("vr_render_rays: ..." etc.) where the C call refuses its arguments.
#pragma once
#include <cstdint>

#include "volrend/renderer_kernel.hpp"
#include "volrend/weights.hpp"

namespace volrend {

// n rays: device, float32 [n][3] each, world space; a direction may have any finite non-zero length.  Ray i is
// the ray of a pixel entered behind screen2worlddir's matrix product, marched as an offscreen frame without
// mesh depth: a list built from a camera gives that frame's bits.  64 consecutive rays share a wave; the
// library does not reorder them (order_rays below computes an order for the caller to apply).
struct Rays {
    const float* origins = nullptr;
    const float* dirs = nullptr;
    int64_t n = 0;
};

//   rgba   device, [n] RGBA8: the composite over background_brightness;  accum  device, float32 [n][4]:
//   trace_ray's output before the composite.  nullptr = not wanted, at least one.  render_depth and
//   enable_probe are refused.
void render_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options, void* rgba, float* accum,
                 void* stream, int fp_mode = VR_FP_STRICT);

// accumulate_weights (weights.hpp) over the rays of a list; no ray: only the file-order table is uploaded.
void accumulate_weights_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options,
                             const LeafWeights& out, void* stream, int fp_mode = VR_FP_STRICT);

// render_backward (grad.hpp) over the rays of a list: grad_accum is float32 [n][4], row i for ray i.
void render_backward_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options,
                          const float* grad_accum, float* grad_data, void* stream, int fp_mode = VR_FP_STRICT);

// The same, marking the slots it adds into in `touched` (grad.hpp; vr_render_backward_rays_touched).
void render_backward_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options,
                          const float* grad_accum, float* grad_data, uint32_t* touched, void* stream,
                          int fp_mode = VR_FP_STRICT);

// The L2 loss of the rays against target colours and its gradient with respect to the tree, in one launch
// (vr_fit_rays): what render_rays (accum), the composite over background_brightness, the residual and the marked
// render_backward_rays compute in sequence.  The loss is grad_scale / 2 * sum r^2 over rays and channels.
struct Fit {
    const float* target = nullptr;  // device, float32 [n][3]: the colour ray i should have
    float grad_scale = 0.f;         // finite; 2 / (3 n) for the mean
    float* grad_data = nullptr;     // as render_backward_rays: added into, required
    uint32_t* touched = nullptr;    // ORed into; nullptr = not wanted
    float* sq_err = nullptr;        // [n]: the squared residual of ray i summed over channels; nullptr = not wanted
    float* accum = nullptr;         // [n][4]: the bits render_rays gives; nullptr = not wanted
};
void fit_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options, const Fit& fit, void* stream,
              int fp_mode = VR_FP_STRICT);

// The order that makes a ray list coherent, and the list gathered into it (vr_order_rays; include/volrend_hip.h
// has the key and the result rule).  order_out[j] = the index of the ray at sorted position j (a stable sort:
// unique and bit-reproducible); the march calls above then take origins_out / dirs_out / payload_out, and per-ray
// outputs go back to the caller's order through order_out.  The caller owns the workspace
// (order_rays_workspace(n) bytes, 256-byte aligned).  No launch slot: safe beside any launch.
struct RayOrder {
    int bits = 0;                    // 1..5 key bits per coordinate; 0 = the library's default
    uint32_t* order = nullptr;       // device, [n], required
    uint32_t* keys = nullptr;        // device, [n]: the sorted keys; nullptr = not wanted
    float* origins_out = nullptr;    // device, [n][3]; nullptr = not wanted
    float* dirs_out = nullptr;       // device, [n][3], as given (not normalised); nullptr = not wanted
    const float* payload = nullptr;  // device, [n][payload_dim], e.g. Fit::target; nullptr = none
    float* payload_out = nullptr;    // required iff payload
    int payload_dim = 0;             // 1..8 with a payload
};
size_t order_rays_workspace(int64_t n);
void order_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options, const RayOrder& out,
                void* workspace, size_t workspace_bytes, void* stream, int fp_mode = VR_FP_STRICT);

// Sizes n_slots launch slots so that no later ray call of <= n rays on them allocates (vr_reserve_rays).
void reserve_rays(const N3Tree& tree, int64_t n, int n_slots = 2);

}  // namespace volrend
