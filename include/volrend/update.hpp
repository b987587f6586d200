// volrend::update_data / read_data -- the values of an uploaded tree written in place and read back, over
// the HIP C ABI (vr_tree_update_data / vr_tree_read_data, include/volrend_hip.h, which has the contract).
// The step that follows render_backward in an optimiser loop (apply the gradient to fp32 master parameters,
// then update_data), and the way to seed or save those parameters from the device; the reference renderer,
// whose tree is read-only, has no counterpart.
// Asynchronous like launch_renderer: both return after enqueueing on `stream` (a hipStream_t passed as
// void*); they throw std::runtime_error ("vr_tree_update_data: ..." / "vr_tree_read_data: ...") where the C
// call refuses its arguments.
#pragma once
#include "volrend/n3tree.hpp"

namespace volrend {

enum class DataType : int { F16 = VR_DATA_F16, F32 = VR_DATA_F32 };

// data_dev: device memory on the tree's device, capacity * N^3 * data_dim elements of `dtype`, indexed like the
// file's data array (the file's node numbering, record [R.., G.., B.., sigma]).
// update_data WRITES the device copy of the tree (F32 is rounded to binary16 to nearest even): launches,
// queries and clones enqueued later on the same stream see the new values, work on other streams has to be
// ordered with events, and nothing may read the tree while the update runs.  Afterwards the device copy is
// bit for bit what an upload of the same child array with this data would have built.  The host arrays of
// `tree` (data_) are not touched: they go stale.
void update_data(const N3Tree& tree, const void* data_dev, DataType dtype, void* stream);

// Writes the tree's current values to data_dev: the bits that were uploaded or last written, the sigma of
// internal slots as +0; F32 is the exact widening.  Only reads the tree.
void read_data(const N3Tree& tree, void* data_dev, DataType dtype, void* stream);

}  // namespace volrend
