// step.cpp -- volrend::tree_step over vr_tree_step.
#include "volrend/step.hpp"

#include "volrend/internal/check.hpp"

namespace volrend {

void tree_step(const N3Tree& tree, const Step& step, void* stream) {
    VrStep s{};
    s.master = step.master;
    s.grad = step.grad;
    s.touched = step.touched;
    s.m = step.m;
    s.v = step.v;
    s.kind = (int32_t)step.kind;
    s.lr = step.lr;
    s.lr_sigma = step.lr_sigma;
    s.beta1 = step.beta1;
    s.beta2 = step.beta2;
    s.eps = step.eps;
    s.step = step.step;
    internal::vr_check(vr_tree_step(tree.device, &s, stream), "vr_tree_step");
}

}  // namespace volrend
