// update.cpp -- volrend::update_data / read_data over vr_tree_update_data / vr_tree_read_data.
#include "volrend/update.hpp"

#include "volrend/internal/check.hpp"

namespace volrend {

void update_data(const N3Tree& tree, const void* data_dev, DataType dtype, void* stream) {
    internal::vr_check(vr_tree_update_data(tree.device, data_dev, (int)dtype, stream), "vr_tree_update_data");
}

void read_data(const N3Tree& tree, void* data_dev, DataType dtype, void* stream) {
    internal::vr_check(vr_tree_read_data(tree.device, data_dev, (int)dtype, stream), "vr_tree_read_data");
}

}  // namespace volrend
