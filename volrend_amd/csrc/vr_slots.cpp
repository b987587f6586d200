// vr_slots.cpp -- the launch-slot ring (LaunchSlot, vr_host.h): picking and growing the slot of a launch, a
// launch's turn at it, and vr_reserve / vr_reserve_tiles / vr_reserve_rays, which size slots up front.
#include <hip/hip_runtime.h>

#include <mutex>

#include "vr_host.h"

namespace {

// Replaces the ray buffer of a slot the caller owns (it holds the launch mutex, or has marked the
// slot `growing` and dropped it) by one of `bytes`.  The slot's last launch must have finished
// before its buffer goes; if that wait fails the buffer is still freed (hipFree synchronises by
// itself): only a failing allocation fails, and nothing is leaked either way.
hipError_t replace_ray_buffer(LaunchSlot& ls, size_t bytes) {
    if (ls.rays) {
        if (ls.used) (void)hipEventSynchronize(ls.done.get());
        (void)ls.rays.reset();
        (void)hipGetLastError();
    }
    return ls.rays.alloc(bytes);
}

// vr_reserve_tiles / vr_reserve_rays: the ray buffers of the first n_slots slots hold `need` bytes.
int reserve_slots(VrTreeOpaque* t, int n_slots, size_t need) {
    DeviceGuard device_guard(t->device);
    std::lock_guard<std::mutex> guard(t->launch_mutex);
    for (int i = 0; i < n_slots; ++i) {
        LaunchSlot& ls = t->slots[i];
        if (ls.growing || ls.rays.bytes() >= need) continue;
        const hipError_t e = replace_ray_buffer(ls, need);
        if (e != hipSuccess) return fail(hip_code(e), "ray buffer of %zu bytes: %s", need, hipGetErrorString(e));
    }
    return VR_OK;
}

// the colour records of a launch of this tree: the largest a ray gets (vr_internal.h)
size_t colour_record_bytes(const VrTreeOpaque* t, uint32_t total_rays) {
    const int flavour = vr::basis_flavour(t->desc.format, t->desc.basis_dim);
    return ray_buffer_bytes(total_rays, vr::kRayWords + vr::ray_tail_words(t->desc.format, flavour));
}

}  // namespace

int acquire_slot(VrTreeOpaque* t, std::unique_lock<std::mutex>& guard, hipStream_t hs, vr::KParams& k,
                 size_t need, unsigned& slot) {
    for (;;) {
        slot = kLaunchSlots;
        for (int want_fit = 1; want_fit >= 0 && slot == kLaunchSlots; --want_fit) {
            for (int pass = 0; pass < 2 && slot == kLaunchSlots; ++pass)
                for (unsigned i = 0; i < kLaunchSlots; ++i) {
                    const LaunchSlot& c = t->slots[i];
                    if (c.growing || (want_fit && c.rays.bytes() < need)) continue;
                    const bool ok = pass == 0 ? (c.used && c.last_stream == hs)
                                              : (!c.used || hipEventQuery(c.done.get()) == hipSuccess);
                    if (ok) {
                        slot = i;
                        break;
                    }
                }
        }
        (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady is an answer, not an error
        // all busy elsewhere: queue up behind one (not one that is growing)
        for (unsigned a = 0; a < kLaunchSlots && slot == kLaunchSlots; ++a)
            if (!t->slots[(t->launch_seq + a) % kLaunchSlots].growing) slot = (t->launch_seq + a) % kLaunchSlots;
        if (slot != kLaunchSlots) break;
        // Every slot is being resized by another thread: wait (the mutex is dropped meanwhile) until one of
        // them is done, then choose again by the same rules.
        t->slot_grown.wait(guard, [t] {
            for (const LaunchSlot& c : t->slots)
                if (!c.growing) return true;
            return false;
        });
    }
    t->launch_seq++;
    LaunchSlot& ls = t->slots[slot];
    k.frames = t->slot_frames.get<vr::FrameDesc>() + (size_t)slot * vr::kMaxBatch;
    k.queue_head = t->slot_heads.get<uint32_t>() + vr::kSlotWords * slot + vr::kSlotHeaderWords;
    k.probe_coeffs = t->probe_buf.get<float>() + (size_t)slot * (size_t)t->desc.data_dim;
    if (ls.rays.bytes() < need) {
        // First use of the slot, or a larger batch than any before: (re)allocate.  This is the
        // one place where an enqueue-only call may block -- on THIS slot's previous launch
        // only, and hipFree/hipMalloc may synchronise the device; vr_reserve() / vr_reserve_tiles()
        // move it out of the render loop.
        // The wait, the free and the allocation run WITHOUT the launch mutex: the slot is marked
        // `growing` (nobody else picks it) and other threads keep enqueueing on the other slots.
        ls.growing = true;
        guard.unlock();
        const hipError_t ge = replace_ray_buffer(ls, need);
        guard.lock();
        ls.growing = false;
        t->slot_grown.notify_all();  // (success or failure: the slot can be picked again)
        if (ge != hipSuccess)
            return fail(hip_code(ge), "ray buffer of %zu bytes: %s", need, hipGetErrorString(ge));
    }
    k.ray_buf_rw = ls.rays.get<uint32_t>();
    k.ray_buf = k.ray_buf_rw;
    return VR_OK;
}

int SlotTurn::begin(LaunchSlot& ls, hipStream_t hs) {
    if (ls.used) HIP_TRY(hipStreamWaitEvent(hs, ls.done.get(), 0));
    slot_ = &ls;
    stream_ = hs;
    return VR_OK;
}

SlotTurn::~SlotTurn() {
    if (!slot_) return;
    if (hipEventRecord(slot_->done.get(), stream_) == hipSuccess) {
        slot_->used = true;
        slot_->last_stream = stream_;
    } else {
        (void)hipGetLastError();
    }
}

extern "C" {

// the slots sized for the largest ray call of n rays: colour records plus the pixel words of a call without rgba
int vr_reserve_rays(vr_tree_t t, int64_t n, int n_slots) {
    if (!t) return fail(VR_ERR_INVALID_ARGUMENT, "vr_reserve_rays: tree is NULL");
    if (n_slots < 1 || n_slots > (int)kLaunchSlots)
        return fail(VR_ERR_INVALID_ARGUMENT, "vr_reserve_rays: n_slots=%d outside [1,%u]", n_slots, kLaunchSlots);
    vr::KParams geo;
    if (int rc = list_geometry("vr_reserve_rays", n, geo)) return rc;
    return reserve_slots(t, n_slots, colour_record_bytes(t, geo.total_rays) + list_pixel_bytes(geo.total_rays));
}

int vr_reserve_tiles(vr_tree_t t, int width, int height, int n_frames, int tile_w, int tile_h,
                     int world, int n_slots) {
    if (!t) return fail(VR_ERR_INVALID_ARGUMENT, "tree is NULL");
    if (n_frames < 1 || n_frames > VR_MAX_BATCH)
        return fail(VR_ERR_INVALID_ARGUMENT, "vr_reserve(%d x %d, %d frames) out of range", width,
                    height, n_frames);
    if (n_slots < 1 || n_slots > (int)kLaunchSlots)
        return fail(VR_ERR_INVALID_ARGUMENT, "n_slots=%d outside [1,%u]", n_slots, kLaunchSlots);
    // exactly the ray count vr_render_batch computes, for rank 0 (which holds the most tiles)
    vr::KParams geo;
    if (int rc = launch_geometry(width, height, tile_w, tile_h, 0, world, n_frames, geo)) return rc;
    // (behind the records: the block masks of such a launch, vr_internal.h "Block cull")
    return reserve_slots(t, n_slots, colour_record_bytes(t, geo.total_rays) + (t->occ ? block_mask_bytes(geo, n_frames) : 0));
}

// two slots of whole frames: what a render loop on one stream (one slot) or on two alternating
// streams needs
int vr_reserve(vr_tree_t t, int width, int height, int n_frames) {
    return vr_reserve_tiles(t, width, height, n_frames, 0, 0, 1, 2);
}

}  // extern "C"
