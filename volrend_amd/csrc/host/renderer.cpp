// renderer.cpp -- volrend::launch_renderer[_aov] over vr_render / vr_render_batch / vr_render_aov, and
// volrend::accumulate_weights / render_backward over vr_accumulate_weights / vr_render_backward (the same
// poses, cameras and options).
#include <stdexcept>
#include <string>

#include "volrend/aov.hpp"
#include "volrend/grad.hpp"
#include "volrend/internal/check.hpp"
#include "volrend/rays.hpp"
#include "volrend/renderer_kernel.hpp"
#include "volrend/weights.hpp"

namespace volrend {
namespace {

VrRenderOptions to_c(const RenderOptions& o) {
    VrRenderOptions c;
    vr_default_options(&c);
    c.step_size = o.step_size;
    c.sigma_thresh = o.sigma_thresh;
    c.stop_thresh = o.stop_thresh;
    c.background_brightness = o.background_brightness;
    for (int i = 0; i < 6; ++i) c.render_bbox[i] = o.render_bbox[i];
    c.basis_minmax[0] = o.basis_minmax[0];
    c.basis_minmax[1] = o.basis_minmax[1];
    for (int i = 0; i < 3; ++i) {
        c.rot_dirs[i] = o.rot_dirs[i];
        c.probe[i] = o.probe[i];
    }
    c.show_grid = o.show_grid;
    c.grid_max_depth = o.grid_max_depth;
    c.render_depth = o.render_depth;
    c.enable_probe = o.enable_probe;
    c.probe_disp_size = o.probe_disp_size;
    return c;
}

VrCamera to_c(const Camera& cam, const float* transform12) {
    VrCamera c;
    for (int i = 0; i < 12; ++i) c.transform[i] = transform12[i];
    c.width = cam.width;
    c.height = cam.height;
    c.fx = cam.fx;
    c.fy = cam.fy;
    return c;
}

VrAov to_c(const AovPlanes& a) {
    VrAov c;
    c.depth = a.depth;
    c.transmittance = a.transmittance;
    c.pitch = a.pitch;
    return c;
}

VrFrame frame_to_c(void* image_rgba8_dev, const float* depth_dev, bool offscreen) {
    VrFrame f;
    vr_default_frame(&f);
    f.rgba = image_rgba8_dev;
    f.depth = depth_dev;
    f.offscreen = offscreen ? 1 : 0;
    return f;
}

// The poses in chunks of VR_MAX_BATCH, as cameras: launch(first, n, cams) once per chunk.
template <class Launch>
void for_camera_chunks(const Camera& cam, const std::vector<const float*>& transforms, Launch&& launch) {
    for (size_t first = 0; first < transforms.size(); first += VR_MAX_BATCH) {
        const int n = (int)std::min<size_t>(VR_MAX_BATCH, transforms.size() - first);
        VrCamera cams[VR_MAX_BATCH];
        for (int i = 0; i < n; ++i) cams[i] = to_c(cam, transforms[first + i]);
        launch(first, n, cams);
    }
}

// One launch per VR_MAX_BATCH poses: vr_render_batch, or with planes (one per pose) vr_render_aov.
void render_batch(const N3Tree& tree, const Camera& cam, const std::vector<const float*>& transforms,
                  const RenderOptions& options, const std::vector<void*>& images,
                  const std::vector<AovPlanes>* aovs, DepthUnits depth_units, void* stream, bool offscreen) {
    const VrRenderOptions o = to_c(options);
    for_camera_chunks(cam, transforms, [&](size_t first, int n, const VrCamera* cams) {
        VrFrame frames[VR_MAX_BATCH];
        std::vector<VrAov> planes(aovs ? (size_t)n : 0);
        for (int i = 0; i < n; ++i) {
            frames[i] = frame_to_c(images[first + i], nullptr, offscreen);
            if (aovs) planes[(size_t)i] = to_c((*aovs)[first + i]);
        }
        if (aovs)
            internal::vr_check(vr_render_aov(tree.device, n, cams, &o, frames, planes.data(), (int)depth_units, stream),
                               "vr_render_aov");
        else
            internal::vr_check(vr_render_batch(tree.device, n, cams, &o, frames, stream), "vr_render_batch");
    });
}

}  // namespace

void launch_renderer(const N3Tree& tree, const Camera& cam, const RenderOptions& options,
                     void* image_rgba8_dev, const float* depth_dev, void* stream, bool offscreen) {
    const VrCamera c = to_c(cam, glm::value_ptr(cam.transform));
    const VrRenderOptions o = to_c(options);
    const VrFrame f = frame_to_c(image_rgba8_dev, depth_dev, offscreen);
    internal::vr_check(vr_render(tree.device, &c, &o, &f, stream), "vr_render");
}

void launch_renderer_batch(const N3Tree& tree, const Camera& cam,
                           const std::vector<const float*>& transforms,
                           const RenderOptions& options, const std::vector<void*>& images,
                           void* stream, bool offscreen) {
    if (transforms.size() != images.size())
        throw std::invalid_argument("launch_renderer_batch: one image per pose");
    render_batch(tree, cam, transforms, options, images, nullptr, DepthUnits{}, stream, offscreen);
}

void accumulate_weights(const N3Tree& tree, const Camera& cam, const std::vector<const float*>& transforms,
                        const RenderOptions& options, const LeafWeights& out, void* stream, int fp_mode) {
    const VrRenderOptions o = to_c(options);
    const auto launch = [&](size_t, int n, const VrCamera* cams) {
        internal::vr_check(vr_accumulate_weights(tree.device, n, cams, &o, fp_mode, &out, stream),
                           "vr_accumulate_weights");
    };
    if (transforms.empty()) launch(0, 0, nullptr);  // (no pose at all: one call with n = 0, the warm-up)
    else for_camera_chunks(cam, transforms, launch);
}

void render_backward(const N3Tree& tree, const Camera& cam, const std::vector<const float*>& transforms,
                     const RenderOptions& options, const float* grad_accum, float* grad_data, void* stream,
                     int fp_mode) {
    const VrRenderOptions o = to_c(options);
    const size_t frame_floats = (size_t)cam.width * (size_t)cam.height * 4;
    const auto launch = [&](size_t first, int n, const VrCamera* cams) {
        internal::vr_check(vr_render_backward(tree.device, n, cams, &o, fp_mode,
                                              grad_accum ? grad_accum + first * frame_floats : nullptr, grad_data,
                                              stream),
                           "vr_render_backward");
    };
    if (transforms.empty()) launch(0, 0, nullptr);  // (no pose at all: one call with n = 0, the warm-up)
    else for_camera_chunks(cam, transforms, launch);
}

void render_backward(const N3Tree& tree, const Camera& cam, const std::vector<const float*>& transforms,
                     const RenderOptions& options, const float* grad_accum, float* grad_data, uint32_t* touched,
                     void* stream, int fp_mode) {
    const VrRenderOptions o = to_c(options);
    const size_t frame_floats = (size_t)cam.width * (size_t)cam.height * 4;
    const auto launch = [&](size_t first, int n, const VrCamera* cams) {
        internal::vr_check(vr_render_backward_touched(tree.device, n, cams, &o, fp_mode,
                                                      grad_accum ? grad_accum + first * frame_floats : nullptr,
                                                      grad_data, touched, stream),
                           "vr_render_backward_touched");
    };
    if (transforms.empty()) launch(0, 0, nullptr);
    else for_camera_chunks(cam, transforms, launch);
}

void render_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options, void* rgba, float* accum,
                 void* stream, int fp_mode) {
    const VrRenderOptions o = to_c(options);
    const VrRays r{rays.origins, rays.dirs};
    const VrRayOut out{rgba, accum};
    internal::vr_check(vr_render_rays(tree.device, rays.n, &r, &o, fp_mode, &out, stream), "vr_render_rays");
}

void accumulate_weights_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options,
                             const LeafWeights& out, void* stream, int fp_mode) {
    const VrRenderOptions o = to_c(options);
    const VrRays r{rays.origins, rays.dirs};
    internal::vr_check(vr_accumulate_weights_rays(tree.device, rays.n, &r, &o, fp_mode, &out, stream),
                       "vr_accumulate_weights_rays");
}

void render_backward_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options,
                          const float* grad_accum, float* grad_data, void* stream, int fp_mode) {
    const VrRenderOptions o = to_c(options);
    const VrRays r{rays.origins, rays.dirs};
    internal::vr_check(vr_render_backward_rays(tree.device, rays.n, &r, &o, fp_mode, grad_accum, grad_data, stream),
                       "vr_render_backward_rays");
}

void render_backward_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options,
                          const float* grad_accum, float* grad_data, uint32_t* touched, void* stream, int fp_mode) {
    const VrRenderOptions o = to_c(options);
    const VrRays r{rays.origins, rays.dirs};
    internal::vr_check(vr_render_backward_rays_touched(tree.device, rays.n, &r, &o, fp_mode, grad_accum, grad_data,
                                                       touched, stream),
                       "vr_render_backward_rays_touched");
}

void fit_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options, const Fit& fit, void* stream,
              int fp_mode) {
    const VrRenderOptions o = to_c(options);
    const VrRays r{rays.origins, rays.dirs};
    const VrFit f{fit.target, fit.grad_scale, fit.grad_data, fit.touched, fit.sq_err, fit.accum};
    internal::vr_check(vr_fit_rays(tree.device, rays.n, &r, &o, fp_mode, &f, stream), "vr_fit_rays");
}

size_t order_rays_workspace(int64_t n) { return (size_t)vr_order_rays_workspace(n); }

void order_rays(const N3Tree& tree, const Rays& rays, const RenderOptions& options, const RayOrder& out,
                void* workspace, size_t workspace_bytes, void* stream, int fp_mode) {
    const VrRenderOptions o = to_c(options);
    const VrRays r{rays.origins, rays.dirs};
    const VrRayOrder ro{out.bits, out.order, out.keys, out.origins_out, out.dirs_out, out.payload, out.payload_out,
                        out.payload_dim};
    internal::vr_check(vr_order_rays(tree.device, rays.n, &r, &o, fp_mode, &ro, workspace, workspace_bytes, stream),
                       "vr_order_rays");
}

void reserve_rays(const N3Tree& tree, int64_t n, int n_slots) {
    internal::vr_check(vr_reserve_rays(tree.device, n, n_slots), "vr_reserve_rays");
}

void launch_renderer_aov(const N3Tree& tree, const Camera& cam, const RenderOptions& options,
                         void* image_rgba8_dev, const float* depth_dev, const AovPlanes& aov,
                         DepthUnits depth_units, void* stream, bool offscreen) {
    const VrCamera c = to_c(cam, glm::value_ptr(cam.transform));
    const VrRenderOptions o = to_c(options);
    const VrAov a = to_c(aov);
    const VrFrame f = frame_to_c(image_rgba8_dev, depth_dev, offscreen);
    internal::vr_check(vr_render_aov(tree.device, 1, &c, &o, &f, &a, (int)depth_units, stream), "vr_render_aov");
}

void launch_renderer_aov_batch(const N3Tree& tree, const Camera& cam,
                               const std::vector<const float*>& transforms, const RenderOptions& options,
                               const std::vector<void*>& images, const std::vector<AovPlanes>& aovs,
                               DepthUnits depth_units, void* stream, bool offscreen) {
    if (transforms.size() != images.size() || transforms.size() != aovs.size())
        throw std::invalid_argument("launch_renderer_aov_batch: one image and one AovPlanes per pose");
    render_batch(tree, cam, transforms, options, images, &aovs, depth_units, stream, offscreen);
}

namespace {
void throw_on_status(uint32_t status) {
    if (status != 0)
        throw std::runtime_error(
            "render status 0x" + std::to_string(status) +
            ": rays hit the sample guard (step_size too small for this scene?): the frames of "
            "these launches are wrong");
}
}  // namespace

void check_render_status(const N3Tree& tree) {
    if (!tree.device) return;
    uint32_t status = 0;
    internal::vr_check(vr_tree_status(tree.device, &status, 1), "vr_tree_status");
    throw_on_status(status);
}

void check_render_status(const N3Tree& tree, void* stream) {
    if (!tree.device) return;
    uint32_t status = 0;
    internal::vr_check(vr_tree_status_on(tree.device, &status, 1, stream), "vr_tree_status_on");
    throw_on_status(status);
}

}  // namespace volrend
