// vr_h2d.h -- host-to-device copies of the tree arrays at link speed: the staged copy pipeline of an
// upload (vr_h2d.cpp).  Host only; nothing here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#pragma GCC visibility push(hidden)

struct CopySegment {
    void* dst;        // device memory of `device`
    const void* src;  // pageable host memory
    size_t bytes;
};

// Copies every segment to `device` and returns when the bytes are there.  32 MB or more in all go
// through the pipeline (several threads, pinned slots, one stream per device); anything smaller, a
// machine with fewer than 4 CPUs, or any failure to set the pipeline up or to run it, takes the plain
// blocking copy.  VR_UPLOAD_TIMING=1 prints a `staged H2D:` line when the pipeline ran.
hipError_t staged_h2d_multi(const CopySegment* seg, int n_seg, int device);

// The pipeline's stream and all its pinned slots for `device` (the current device) up front: the
// first upload of a process pays for them beside its other start-up work.  Best effort.
void warm_upload_cache(int device);

// Maps the pages of a host range of 64 MB or more into this process ahead of the copy that reads
// them.  Blocks until done; best effort, no effect on results.
void prefault_host_range(const void* ptr, size_t bytes);

#pragma GCC visibility pop
