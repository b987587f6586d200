// volrend::tree_step -- a sparse optimiser step over the slots a marked backward call touched, written into the
// uploaded tree in place, over the HIP C ABI (vr_tree_step, include/volrend_hip.h, which has the arithmetic and
// the contract).  With render_rays and the marked render_backward_rays (rays.hpp) it is one iteration of an
// optimiser loop whose cost follows the rays and the leaves they hit, not the size of the tree; the reference
// renderer, whose tree is read-only, has no counterpart.
// Asynchronous like launch_renderer: returns after enqueueing on `stream` (a hipStream_t passed as void*);
// throws std::runtime_error ("vr_tree_step: ...") where the C call refuses its arguments.
#pragma once
#include <cstddef>
#include <cstdint>

#include "volrend/n3tree.hpp"

namespace volrend {

enum class StepKind : int { SGD = VR_STEP_SGD, Adam = VR_STEP_ADAM };

// Device memory on the tree's device.  master / grad / m / v: float32, capacity * N^3 * data_dim elements,
// indexed like the file's data array; touched: touched_words(tree) words, one bit per child slot (bit s & 31 of
// word s >> 5, s = file node * N^3 + child slot), as the marked backward calls set them.
struct Step {
    float* master = nullptr;     // the values the tree's binary16 are rounded from
    float* grad = nullptr;       // read, then set to +0 in every touched slot
    uint32_t* touched = nullptr; // read, then cleared
    float* m = nullptr;          // Adam moments; nullptr for SGD
    float* v = nullptr;
    StepKind kind = StepKind::SGD;
    float lr = 0.f;
    float lr_sigma = 0.f;        // the rate of the sigma entry of a record
    float beta1 = 0.9f, beta2 = 0.999f, eps = 1e-8f;
    int step = 1;                // Adam: 1, 2, ... for the bias correction
};

// Words of a `touched` bitmap of this tree: ceil(capacity * N^3 / 32).
inline size_t touched_words(const N3Tree& tree) {
    return ((size_t)tree.capacity * tree.N * tree.N * tree.N + 31) / 32;
}

// WRITES the device copy of the tree (as update_data does, and ordered like it): in every touched slot master
// moves by the optimiser's rule, the tree takes binary16(master), grad becomes +0; then the bitmap is zero.
// Slots whose bit is clear are neither read nor written.  The host arrays of `tree` go stale.
void tree_step(const N3Tree& tree, const Step& step, void* stream);

}  // namespace volrend
