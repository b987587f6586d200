// volrend::internal owners of HIP resources -- the one rule for the host code of libvolrend_hip.so
// (volrend_amd/csrc/vr_host.h) and the C++ host layer (volrend_amd/csrc/host).  Host only, header
// only.  An owner remembers the device that was current when it created its resource and releases
// the resource with that device current, whatever device the calling thread has then.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace volrend {
namespace internal {

// Makes `device` current for its scope and restores the thread's device afterwards.  A negative
// device (nothing created yet) does nothing: hipSetDevice(-1) would fail, and a failed call leaves
// an error that the next hipGetLastError() reports.
class DeviceGuard {
   public:
    explicit DeviceGuard(int device) {
        if (device >= 0 && hipGetDevice(&prev_) == hipSuccess && prev_ != device)
            switched_ = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched_) (void)hipSetDevice(prev_); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;

   private:
    int prev_ = 0;
    bool switched_ = false;
};

// The one owner of a handle that `Release` frees (move-only).
template <class H, hipError_t (*Release)(H)>
class HipOwner {
   public:
    HipOwner() = default;
    HipOwner(HipOwner&& o) noexcept : h_(std::exchange(o.h_, nullptr)), device_(o.device_) {}
    ~HipOwner() { (void)reset(); }
    hipError_t reset() {
        if (!h_) return hipSuccess;
        DeviceGuard on(device_);
        return Release(std::exchange(h_, nullptr));
    }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }

   protected:
    // Frees what it held, then `create(&handle)` on the current device.
    template <class Create>
    hipError_t acquire(Create create) {
        (void)reset();
        if (hipGetDevice(&device_) != hipSuccess) device_ = -1;
        const hipError_t e = create(&h_);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }

   private:
    H h_ = nullptr;
    int device_ = -1;
};

// Device memory and its size.
class DeviceBuffer : public HipOwner<void*, hipFree> {
   public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : HipOwner(std::move(o)), bytes_(std::exchange(o.bytes_, 0)) {}
    hipError_t alloc(size_t bytes) {
        const hipError_t e = acquire([&](void** p) { return hipMalloc(p, bytes); });
        bytes_ = e == hipSuccess ? bytes : 0;
        return e;
    }
    hipError_t reset() {
        bytes_ = 0;
        return HipOwner::reset();
    }
    template <class T = void>
    T* get() const { return static_cast<T*>(HipOwner::get()); }
    size_t bytes() const { return bytes_; }

   private:
    size_t bytes_ = 0;
};

// Page-locked host memory.
class PinnedBuffer : public HipOwner<void*, hipHostFree> {
   public:
    hipError_t alloc(size_t bytes) {
        return acquire([&](void** p) { return hipHostMalloc(p, bytes, hipHostMallocDefault); });
    }
    template <class T = void>
    T* get() const { return static_cast<T*>(HipOwner::get()); }
};

class DeviceEvent : public HipOwner<hipEvent_t, hipEventDestroy> {
   public:
    hipError_t create(unsigned flags = hipEventDisableTiming) {
        return acquire([&](hipEvent_t* e) { return hipEventCreateWithFlags(e, flags); });
    }
};

class DeviceStream : public HipOwner<hipStream_t, hipStreamDestroy> {
   public:
    hipError_t create(unsigned flags) {
        return acquire([&](hipStream_t* s) { return hipStreamCreateWithFlags(s, flags); });
    }
};

}  // namespace internal
}  // namespace volrend
