// quantize.cpp -- volrend::quantize over vr_quantize.
#include "volrend/quantize.hpp"

#include <stdexcept>
#include <string>

#include "volrend/internal/check.hpp"

namespace volrend {

int64_t quantize_workspace(int64_t n_slots, int data_dim) {
    const int64_t bytes = vr_quantize_workspace(n_slots, data_dim);
    if (bytes < 0)
        throw std::runtime_error("vr_quantize_workspace: n_slots = " + std::to_string(n_slots) + ", data_dim = " +
                                 std::to_string(data_dim) + " are refused");
    return bytes;
}

void quantize(const Quantize& q, void* stream) {
    VrQuantize c{};
    c.data = q.data;
    c.quant_colors = q.quant_colors;
    c.quant_map = q.quant_map;
    c.sigma = q.sigma;
    c.data_retained = q.data_retained;
    c.workspace = q.workspace;
    c.workspace_bytes = q.workspace_bytes;
    c.n_slots = q.n_slots;
    c.data_dim = q.data_dim;
    c.n_retained = q.n_retained;
    c.bits = q.bits;
    c.sigma_thresh = q.sigma_thresh;
    internal::vr_check(vr_quantize(&c, stream), "vr_quantize");
}

}  // namespace volrend
