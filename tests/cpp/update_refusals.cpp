// update_refusals.cpp -- the refusals of volrend::update_data / read_data (include/volrend/update.hpp), which
// need no device: every check below comes before the tree handle is followed, so the tree carries a handle
// that is never followed and the data pointer is never read or written.  Prints one line per case:
// "<case> <what()>".
#include <cstdio>
#include <stdexcept>
#include "volrend/update.hpp"
using namespace volrend;
template <typename F> static void expect_throw(const char* name, F&& f) {
    try { f(); std::printf("%s NO_THROW\n", name); }
    catch (const std::runtime_error& e) { std::printf("%s runtime_error: %s\n", name, e.what()); }
}
int main() {
    N3Tree tree, none;   // `none` has no device copy: its handle is NULL
    tree.device = reinterpret_cast<vr_tree_t>(0x1000);  // never followed: every call below is refused first
    void* d = reinterpret_cast<void*>(0x5000);
    expect_throw("update_null_tree", [&] { update_data(none, d, DataType::F16, nullptr); });
    expect_throw("update_null_data", [&] { update_data(tree, nullptr, DataType::F32, nullptr); });
    expect_throw("update_dtype", [&] { update_data(tree, d, static_cast<DataType>(2), nullptr); });
    expect_throw("read_null_tree", [&] { read_data(none, d, DataType::F32, nullptr); });
    expect_throw("read_null_data", [&] { read_data(tree, nullptr, DataType::F16, nullptr); });
    expect_throw("read_dtype", [&] { read_data(tree, d, static_cast<DataType>(-1), nullptr); });
    tree.device = nullptr;
    return 0;
}
