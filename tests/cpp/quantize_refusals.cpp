// quantize_refusals.cpp -- the refusals of volrend::quantize / quantize_workspace (include/volrend/quantize.hpp),
// which need no device: every check below comes before any device call, so the pointers are never read or written.
// Prints one line per case: "<case> <what()>".
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include "volrend/quantize.hpp"
using namespace volrend;
template <typename F> static void expect_throw(const char* name, F&& f) {
    try { f(); std::printf("%s NO_THROW\n", name); }
    catch (const std::runtime_error& e) { std::printf("%s runtime_error: %s\n", name, e.what()); }
}
int main() {
    Quantize q;
    q.data = reinterpret_cast<const uint16_t*>(0x1000);
    q.n_slots = 80;
    q.data_dim = 13;
    q.n_retained = 1;
    q.bits = 5;
    q.quant_colors = reinterpret_cast<uint16_t*>(0x2000);
    q.quant_map = reinterpret_cast<uint16_t*>(0x3000);
    q.sigma = reinterpret_cast<uint16_t*>(0x4000);
    q.data_retained = reinterpret_cast<uint16_t*>(0x5000);
    q.workspace = reinterpret_cast<void*>(0x100000);
    q.workspace_bytes = quantize_workspace(q.n_slots, q.data_dim);
    auto bad = [&](const char* name, auto&& change) {
        Quantize b = q;
        change(b);
        expect_throw(name, [&] { quantize(b, nullptr); });
    };
    bad("null_data", [](Quantize& b) { b.data = nullptr; });
    bad("null_colors", [](Quantize& b) { b.quant_colors = nullptr; });
    bad("null_map", [](Quantize& b) { b.quant_map = nullptr; });
    bad("null_sigma", [](Quantize& b) { b.sigma = nullptr; });
    bad("null_workspace", [](Quantize& b) { b.workspace = nullptr; });
    bad("retained_missing", [](Quantize& b) { b.data_retained = nullptr; });
    bad("retained_unwanted", [](Quantize& b) { b.n_retained = 0; });
    bad("slots_zero", [](Quantize& b) { b.n_slots = 0; });
    bad("slots_large", [](Quantize& b) { b.n_slots = int64_t(1) << 31; });
    bad("dim_small", [](Quantize& b) { b.data_dim = 1; });
    bad("dim_odd", [](Quantize& b) { b.data_dim = 12; });
    bad("retain_negative", [](Quantize& b) { b.n_retained = -1; });
    bad("retain_all", [](Quantize& b) { b.n_retained = 4; });
    bad("bits_zero", [](Quantize& b) { b.bits = 0; });
    bad("bits_large", [](Quantize& b) { b.bits = 17; });
    bad("thresh_nan", [](Quantize& b) { b.sigma_thresh = std::nanf(""); });
    bad("workspace_small", [](Quantize& b) { b.workspace_bytes -= 1; });
    bad("workspace_misaligned", [](Quantize& b) { b.workspace = reinterpret_cast<void*>(0x100080); });
    bad("output_is_input", [](Quantize& b) { b.sigma = const_cast<uint16_t*>(b.data); });
    expect_throw("size_slots", [] { (void)quantize_workspace(0, 13); });
    expect_throw("size_dim", [] { (void)quantize_workspace(80, 14); });
    return 0;
}
