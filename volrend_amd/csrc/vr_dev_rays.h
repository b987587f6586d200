// vr_dev_rays.h -- a ray from pixel to pixel: ray-id order, ray generation up to the ray/box test,
// the compositing tail, the ray buffer raygen_kernel writes and render_kernel reads, and the ray
// queues ray generation compacts its rays into and the persistent waves draw their chunks from, and the front
// of the ray-list launches (list_ray).
// Device code only.
#pragma once
#include "vr_device_math.h"
#include "vr_dev_layout.h"
#include "vr_dev_shade.h"  // quant8

namespace vr {

namespace {

struct RayCounters {
    uint32_t samples = 0, child_reads = 0, hits = 0, early = 0, entered = 0;
};

typedef __attribute__((address_space(1))) uint32_t vr_gword_t;   // a dword of a frame buffer
typedef float vr_f4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) vr_f4_t vr_gfloat4_t;

__device__ __forceinline__ bool wave_any(bool v) { return __builtin_amdgcn_ballot_w64(v) != 0ull; }
// The lane's id, recomputed where it is asked for (two instructions): for addresses that are needed
// once in a while -- a register that holds `lane * 4` across the march loop is one the hot path lacks.
__device__ __forceinline__ uint32_t lane_id_now() {
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
// Number of set bits of a wave mask below this lane: the lane's rank among the lanes of the mask.
__device__ __forceinline__ uint32_t lane_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

struct Ray {
    float cen[3], dir[3], invdir[3];
    float t, tmax, delta_scale;
    float light;
    float out[4];
    bool active;      // lane holds an unfinished ray
    bool alive;       // still inside `while (t < tmax)`
    bool entered;     // passed the ray/box test of rt_core.cuh:88
    bool stopped;     // ended by stop_thresh (renormalised in finish_ray)
};

struct PixelRef {
    int32_t frame, x, y, k, lx, ly;
    bool in_image;
};

__device__ __forceinline__ PixelRef locate(const KParams& p, uint32_t id) {
    PixelRef r;
    // Ray-id order (scheduling only; consecutive ids are generated, queued and marched together):
    // the frames of the launch are taken in groups of p.frame_group consecutive poses; within a
    // group the 8x8 pixel block is the major index and the FRAME the minor one, so the same
    // block of neighbouring poses -- rays that walk through nearly the same leaves -- sits in
    // consecutive ids; the blocks of a tile are visited super-block by super-block
    // (p.super_block x p.super_block blocks, row-major inside), so that a wave's chunk of ids
    // covers a compact screen region instead of a thin strip.
    const uint32_t blk = id >> 6;
    const int32_t lane = (int32_t)(id & 63u);
    const uint32_t G = (uint32_t)p.frame_group, nwb = (uint32_t)p.n_wave_blocks;
    const uint32_t grp = blk / (nwb * G), rem = blk - grp * nwb * G;
    const uint32_t left = (uint32_t)p.n_frames - grp * G, gsz = left < G ? left : G;
    const int32_t wb = (int32_t)(rem / gsz);
    r.frame = (int32_t)(grp * G + (rem - (uint32_t)wb * gsz));
    // wave block -> local tile -> frame tile -> pixel
    r.k = wb / p.wblocks_per_tile;
    const int32_t sub = wb - r.k * p.wblocks_per_tile;
    const int32_t tile = r.k * p.world + p.rank;
    const int32_t ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    int32_t sx, sy;
    const int32_t nbx = p.wblocks_per_tile_x;
    if (p.super_block <= 1) {
        sy = sub / nbx;
        sx = sub - sy * nbx;
    } else {  // ragged edges: the last super-row / super-column is simply shorter
        const int32_t S = p.super_block, nby = p.wblocks_per_tile / nbx;
        const int32_t per_sr = S * nbx, full_sr = nby / S;
        int32_t sr = sub / per_sr, in_sr = sub - sr * per_sr, rows = S;
        if (sr >= full_sr) {
            sr = full_sr;
            in_sr = sub - full_sr * per_sr;
            rows = nby - full_sr * S;
        }
        const int32_t per_sc = rows * S, full_sc = nbx / S;
        int32_t sc = in_sr / per_sc, in_sc = in_sr - sc * per_sc, cols = S;
        if (sc >= full_sc) {
            sc = full_sc;
            in_sc = in_sr - full_sc * per_sc;
            cols = nbx - full_sc * S;
        }
        const int32_t iy = in_sc / cols;
        sx = sc * S + (in_sc - iy * cols);
        sy = sr * S + iy;
    }
    r.lx = sx * 8 + (lane & 7);
    r.ly = sy * 8 + (lane >> 3);
    r.x = tx * p.tile_w + r.lx;
    r.y = ty * p.tile_h + r.ly;
    r.in_image = r.x < p.width && r.y < p.height;
    return r;
}

// The RGBA8 of frame pixel (x, y) = pixel (lx, ly) of the rank's k-th tile.
__device__ __forceinline__ uint8_t* pixel_address(const KParams& p, const FrameDesc& fd, int k, int lx,
                                                  int ly, int x, int y) {
    if (p.layout == VR_LAYOUT_COMPACT)
        return fd.rgba + ((int64_t)k * p.tile_w * p.tile_h + (int64_t)ly * p.tile_w + lx) * 4;
    return fd.rgba + (int64_t)y * p.pitch + (int64_t)x * 4;
}
__device__ __forceinline__ uint8_t* pixel_ptr(const KParams& p, const FrameDesc& fd,
                                              const PixelRef& r) {
    return pixel_address(p, fd, r.k, r.lx, r.ly, r.x, r.y);
}

// A ray from (cen, dir) on: world-space origin and NORMALISED world-space direction -- where screen2worlddir
// (volrend.cu:22-32) leaves a pixel's ray -- through maybe_world2ndc, the world->tree transform, the
// view-direction rotation, _get_delta_scale and the ray/box test (volrend.cu:34-71, rt_core.cuh:52-92).
// The tail of setup_ray, and all of a caller-supplied ray (vr_render_rays: list_ray below).  vdir = the (rotated)
// view direction for the basis; tmax_of() = the ray's far limit before the division by delta_scale (a
// pixel's mesh depth; 1e9 without one), asked where the pixel's ray asks it.
template <int FMA, typename TmaxOf>
__device__ __forceinline__ void setup_ray_from(const KParams& p, float* cen, float* dir, Ray& ray, float* vdir,
                                               TmaxOf&& tmax_of) {
    using P = Policy<FMA>;
    vdir[0] = dir[0];
    vdir[1] = dir[1];
    vdir[2] = dir[2];
    if (p.ndc_width > 0) {  // maybe_world2ndc, volrend.cu:34-54
        const float tt = -(1.f + cen[2]) / dir[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) cen[i] = P::madd(tt, dir[i], cen[i]);
        dir[0] = -((2.f * p.ndc_focal) / p.ndc_width) * (dir[0] / dir[2] - cen[0] / cen[2]);
        dir[1] = -((2.f * p.ndc_focal) / p.ndc_height) * (dir[1] / dir[2] - cen[1] / cen[2]);
        dir[2] = -2.f / cen[2];
        cen[0] = -((2.f * p.ndc_focal) / p.ndc_width) * (cen[0] / cen[2]);
        cen[1] = -((2.f * p.ndc_focal) / p.ndc_height) * (cen[1] / cen[2]);
        cen[2] = 1.f + 2.f / cen[2];
        normalize3<FMA>(dir);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) cen[i] = P::madd(p.scale[i], cen[i], p.offset[i]);

    float tmax_bg = tmax_of();

    if (p.rot_enabled) {  // rodrigues, volrend.cu:57-71 (uniform part done on host)
        float cr[3];
        cross3<FMA>(p.rot_k, vdir, cr);
        const float dot = dot3<FMA>(p.rot_k, vdir);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float a = P::madd(vdir[i], p.rot_cos, cr[i] * p.rot_sin);
            const double kd = (double)(p.rot_k[i] * dot);
            const double om = 1.0 - (double)p.rot_cos;
            vdir[i] = (float)P::dmadd(kd, om, (double)a);
        }
    }
    // _get_delta_scale, rt_core.cuh:52-63
    dir[0] *= p.scale[0];
    dir[1] *= p.scale[1];
    dir[2] *= p.scale[2];
    const float delta_scale = 1.f / norm3<FMA>(dir);
    dir[0] *= delta_scale;
    dir[1] *= delta_scale;
    dir[2] *= delta_scale;
    tmax_bg /= delta_scale;
    float invdir[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) invdir[i] = (float)(1.0 / ((double)dir[i] + 1e-9));
    // _dda_world, rt_core.cuh:18-34: the 1e-6 literals make this FP64
    float tmin = 0.0f, tmax = 1e4f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float t1 = (float)((((double)p.bbox[i] + 1e-6) - (double)cen[i]) * (double)invdir[i]);
        const float t2 =
            (float)((((double)p.bbox[i + 3] - 1e-6) - (double)cen[i]) * (double)invdir[i]);
        tmin = vmax(tmin, vmin(t1, t2));
        tmax = vmin(tmax, vmax(t1, t2));
    }
    tmax = vmin(tmax, tmax_bg);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ray.cen[i] = cen[i];
        ray.dir[i] = dir[i];
        ray.invdir[i] = invdir[i];
    }
    ray.delta_scale = delta_scale;
    ray.tmax = tmax;
    if (tmax < 0 || tmin > tmax) {
        if (p.render_depth) ray.out[3] = 1.f;  // ray misses the box, rt_core.cuh:88-92
        return;
    }
    ray.entered = true;
    ray.t = tmin;
    ray.alive = tmin < tmax;
}

// What every ray starts from (the part of setup_ray in front of enable_draw).
__device__ __forceinline__ void reset_ray(Ray& ray) {
    ray.out[0] = ray.out[1] = ray.out[2] = ray.out[3] = 0.f;
    ray.light = 1.f;
    ray.alive = ray.entered = ray.stopped = false;
    ray.t = 0.f;
}

// Ray generation + trace_ray prologue up to the ray/box test
// (volrend.cu:135-148, rt_core.cuh:74-92).  vdir = (rotated) view direction for the basis.
template <int FMA>
__device__ __forceinline__ void setup_ray(const KParams& p, const PixelRef& r, Ray& ray,
                                          float* vdir) {
    using P = Policy<FMA>;
    const FrameDesc& fd = p.frames[r.frame];
    reset_ray(ray);
    if (p.N <= 0) return;  // enable_draw = tree.N > 0
    float dir[3], cen[3];
    // screen2worlddir, volrend.cu:22-32 (no +0.5 pixel centre offset)
    float xyz[3];
    xyz[0] = P::nmadd(0.5f, (float)p.width, (float)r.x) / p.fx;
    xyz[1] = -(P::nmadd(0.5f, (float)p.height, (float)r.y)) / p.fy;
    xyz[2] = -1.0f;
    float xf[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) xf[i] = fd.xf[i];
    mv3<FMA>(xf, xyz, dir);
    normalize3<FMA>(dir);
    cen[0] = xf[9];
    cen[1] = xf[10];
    cen[2] = xf[11];
    setup_ray_from<FMA>(p, cen, dir, ray, vdir, [&]() -> float {
        float tmax_bg = 1e9f;
        if (!p.offscreen && fd.depth) tmax_bg = fd.depth[(int64_t)r.y * p.width + r.x];
        return tmax_bg;
    });
}

// End of trace_ray + the compositing tail of render_kernel (rt_core.cuh:176-194,
// volrend.cu:152-172): early-stop renormalisation / final alpha, optional debug
// outputs, composite, quantise, store.
// px = the pixel's RGBA8 in its frame buffer; xy (x | y << 16) and frame are only read by the
// optional outputs (accumulators / counters).
template <int FMA, bool COUNT>
__device__ __forceinline__ void finish_ray(const KParams& p, Ray& ray, const RayCounters& rc,
                                           uint8_t* px, uint32_t xy, int frame) {
    using P = Policy<FMA>;
    float* out = ray.out;
    // (COUNT <=> not the FAST flavour: render_depth launches never take FAST, launch_fp)
    float alpha = out[3];  // (0, or 1 for a depth-mode ray that misses the box: ray generation)
    if (ray.stopped) {  // rt_core.cuh:176-185, applied once every queued colour has landed
        if (COUNT && p.render_depth) out[0] = out[1] = out[2] = vmin(out[0] * 0.3f, 1.0f);
        const float scale = 1.f / (1.f - ray.light);
        out[0] *= scale;
        out[1] *= scale;
        out[2] *= scale;
        alpha = 1.f;
    } else if (ray.entered) {  // rt_core.cuh:189-194
        if (COUNT && p.render_depth) {
            out[0] = out[1] = out[2] = vmin(out[0] * 0.3f, 1.0f);
            alpha = 1.f;
        } else {
            alpha = 1.f - ray.light;
        }
    }
    if (COUNT && p.frames[frame].counters) {
        const FrameDesc& fd = p.frames[frame];
        // alg_bytes per SURVEY.md 8(d):
        //   sum over samples (4*L + 2 + hit*2*(data_dim-1)) + 4 per pixel
        const unsigned long long bytes = 4ull * rc.child_reads + 2ull * rc.samples +
                                         2ull * (unsigned long long)(p.data_dim - 1) * rc.hits +
                                         4ull;
        // (the struct is reached through the frame table at every add, not through a local copy of
        // the pointer: that would change the code of every instrumented flavour)
        auto tally = [](uint64_t& word, unsigned long long v) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&word), v);
        };
        if (p.N > 0) tally(fd.counters->rays, 1ull);
        tally(fd.counters->rays_hit_box, ray.entered ? 1ull : 0ull);
        tally(fd.counters->samples, rc.samples);
        tally(fd.counters->child_reads, rc.child_reads);
        tally(fd.counters->hit_samples, rc.hits);
        tally(fd.counters->alg_bytes, bytes);
        tally(fd.counters->early_stops, rc.early);
    }
    if (p.any_accum) {  // launch-uniform: the frame table is only consulted when some frame asks
        float* accum = p.frames[frame].accum;
        if (accum) {
            const int64_t pix = (int64_t)(xy >> 16) * p.width + (int64_t)(xy & 0xFFFFu);
            // (frame buffers are global memory: say so, a pointer read from a table is "flat" to the
            // compiler and would be accessed with flat_ instructions)
            ((vr_gfloat4_t*)accum)[pix] = (vr_f4_t){out[0], out[1], out[2], alpha};
        }
    }
    vr_gword_t* const gpx = (vr_gword_t*)px;
    // composite, volrend.cu:152-172
    const float nalpha = 1.f - alpha;
    if (p.offscreen) {
        out[0] = P::madd(p.background_brightness, nalpha, out[0]);
        out[1] = P::madd(p.background_brightness, nalpha, out[1]);
        out[2] = P::madd(p.background_brightness, nalpha, out[2]);
    } else {
        const uint32_t init = *gpx;
        out[0] = P::madd((float)(init & 0xFFu) / 255.f, nalpha, out[0]);
        out[1] = P::madd((float)((init >> 8) & 0xFFu) / 255.f, nalpha, out[1]);
        out[2] = P::madd((float)((init >> 16) & 0xFFu) / 255.f, nalpha, out[2]);
    }
    *gpx = quant8(out[0]) | (quant8(out[1]) << 8) | (quant8(out[2]) << 16) | 0xFF000000u;
}

// ---------------------------------------------------------------------------
// Ray buffer (global memory, written by raygen_kernel; the words of a ray: kRay*, vr_internal.h).
// ---------------------------------------------------------------------------
// Blocked structure of arrays: the rays are stored in blocks of 64, word k of the 64 rays of a
// block contiguous (256 bytes), the words of a block back to back.  So word k of ray r lives at
//   buf + ((r >> 6) * words_per_ray + k) * 64 + (r & 63)
// -- lanes that hold consecutive rays read / write consecutive dwords, and all the words of one
// ray hang off ONE per-lane address with compile-time offsets (k * 256 bytes: the immediate
// field of the load), so neither address arithmetic nor a base register per field is spent.
template <typename T>
__device__ __forceinline__ T* ray_slot(T* buf, int words_per_ray, uint32_t r) {
    return buf + ((size_t)(r >> 6) * (uint32_t)words_per_ray * 64u + (r & 63u));
}
__device__ __forceinline__ uint32_t ray_word(const uint32_t* slot, int k) { return slot[k * 64]; }
__device__ __forceinline__ uint32_t& ray_word(uint32_t* slot, int k) { return slot[k * 64]; }
constexpr uint32_t kStealMin = 8192;  // rays a foreign queue must still hold to be worth a steal (or an eighth of its length)

// Ray queues.  The 8x8 pixel blocks of a launch (ray-id order: locate()) are cut into n_queues (1 or
// kMaxQueues) contiguous runs -- screen regions of the batch -- at multiples of 16 blocks; queue x owns the ray
// slots of its blocks, [first_block(x) * 64, first_block(x + 1) * 64), and two words of one 64-byte
// line: head (rays handed out, render_kernel) and count (rays stored, raygen_kernel).  Ray generation
// compacts the rays that enter the volume to the front of their queue's region (one atomic on the
// queue's count word per workgroup: eight words share the load a single counter carried, which is
// what lets small launches generate their rays in workgroups of one or four waves: raygen_kernel).
__device__ __forceinline__ uint32_t queue_first_block(uint32_t n_groups16, uint32_t x, uint32_t sh) {
    return (uint32_t)(((uint64_t)n_groups16 * x) >> sh) << 4;
}
// The split of this launch: sh = log2(n_queues), n16 = its groups of 16 blocks.
__device__ __forceinline__ void queue_split(const KParams& p, uint32_t& sh, uint32_t& n16) {
    sh = (uint32_t)p.n_queues == (uint32_t)kMaxQueues ? (uint32_t)kMaxQueuesShift : 0u;
    n16 = ray_groups16(p.total_rays);
}

// A wave's next private range [lo, hi) of ray slots, or lo == hi when there is nothing left for it.
// A wave serves the queue of its XCD first (workgroup b runs on XCD b % 8 -- used for L2 affinity
// only, never for correctness) and steals from the others when that queue has run dry.  Chunk sizes
// shrink as a queue drains (guided self-scheduling) so the tail stays balanced.
//   * One lane walks the queues: one load per queue, and ONE returning atomic on the queue that is
//     picked.  A single word sustains ~90 accesses per microsecond chip-wide (one queue for the
//     whole chip: a one-frame launch takes 40 % longer, profiles/r03_steal_threshold.jsonl).
//   * Waves steal from a queue only while it holds a good part of its rays (an eighth, at most
//     kStealMin); the rest is left to the queue's own waves.  Stealing down to the last chunk
//     -- round 2 -- had every wave of the chip visit every queue when they ran dry, all at
//     about the same time, and scattered the last blocks of every screen region over all
//     XCDs: a one-frame launch marched at a third of its rate for 50 us
//     (profiles/r03_tail_profile.jsonl; without any stealing a 20-frame launch is 5 % slower).
//     A wave only reports "nothing left" after its OWN queue has run dry, so every queue is
//     drained by the waves it belongs to -- which a grid of fewer waves than queues does not
//     have for every queue: such a grid steals to the end.
__device__ __forceinline__ void grab_chunk(const KParams& p, int lane, uint32_t& lo, uint32_t& hi) {
    lo = hi = 0;
    if (lane == 0) {
        const uint32_t nq = (uint32_t)p.n_queues;  // 1 or kMaxQueues
        uint32_t sh, n16;
        queue_split(p, sh, n16);
        const uint32_t mine = blockIdx.x & (nq - 1u);
        const uint32_t waves_per_q = (gridDim.x + nq - 1u) >> sh;
        for (uint32_t a = 0; a < nq; ++a) {
            const uint32_t x = (mine + a) & (nq - 1u);
            uint32_t* const q = p.queue_head + x * kQueueStride;
            uint32_t* const head = q + kQueueHead;
            const uint32_t len = q[kQueueCount];  // rays of this queue (written by raygen_kernel, constant here)
            const uint32_t seen = __hip_atomic_load(head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen >= len) continue;
            if (a != 0u && gridDim.x >= nq &&
                len - seen < ((len >> 3) < kStealMin ? (len >> 3) : kStealMin))
                continue;  // not worth a steal
            uint32_t size = (len - seen) / (2u * waves_per_q);
            size = size < 64u ? 64u : (size > (uint32_t)p.chunk_max ? (uint32_t)p.chunk_max : size);
            size &= ~63u;
            const uint32_t base = atomicAdd(head, size);
            if (base < len) {
                const uint32_t qlo = queue_first_block(n16, x, sh) << 6;
                lo = qlo + base;
                hi = qlo + (base + size < len ? base + size : len);
                break;
            }
        }
    }
}

// Ray generation's compaction (raygen_kernel, march_raygen_kernel; GW = waves per workgroup, every
// lane of the workgroup calls): m_valid = the wave's lanes whose ray enters the volume.  Returns the ray
// slot of the wave's first such lane; the others follow by lane_rank(m_valid).
// Wave ballot + mbcnt prefix inside the wave, a scan over the workgroup's waves, and
// ONE atomic per workgroup on the count word of the queue that owns the workgroup's blocks (a
// single word only sustains ~90 returning atomics per microsecond chip-wide; workgroups never
// straddle a queue boundary: those lie at multiples of 16 blocks).
template <int GW>
__device__ __forceinline__ uint32_t reserve_ray_slots(const KParams& p, unsigned long long m_valid, int lane,
                                                      int wave) {
    __shared__ uint32_t wave_count[GW];
    __shared__ uint32_t wave_base[GW];
    const uint32_t nq = (uint32_t)p.n_queues;
    uint32_t sh, n16;
    queue_split(p, sh, n16);
    const uint32_t g16 = (uint32_t)(((int64_t)blockIdx.x * GW) >> 4);  // this workgroup's group of 16 blocks
    uint32_t qx = (uint32_t)(((uint64_t)g16 << sh) / n16);               // its queue: first guess, then exact
    while (qx + 1u < nq && (queue_first_block(n16, qx + 1u, sh) >> 4) <= g16) ++qx;
    while (qx > 0u && (queue_first_block(n16, qx, sh) >> 4) > g16) --qx;
    uint32_t* const q_count = p.queue_head + qx * kQueueStride + kQueueCount;
    const uint32_t q_base = queue_first_block(n16, qx, sh) << 6;
    if constexpr (GW == 1) {
        const uint32_t n = (uint32_t)__builtin_popcountll(m_valid);
        uint32_t b = 0;
        if (lane == 0 && n) b = atomicAdd(q_count, n);
        return q_base + (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    } else {
        if (lane == 0) wave_count[wave] = (uint32_t)__builtin_popcountll(m_valid);
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t sum = 0;
#pragma unroll
            for (int w = 0; w < GW; ++w) {
                wave_base[w] = sum;
                sum += wave_count[w];
            }
            const uint32_t base = q_base + (sum ? atomicAdd(q_count, sum) : 0u);
#pragma unroll
            for (int w = 0; w < GW; ++w) wave_base[w] += base;
        }
        __syncthreads();
        return wave_base[wave];
    }
}

// ---------------------------------------------------------------------------
// Ray lists (vr_internal.h RayList): the front of raygen_rays_kernel and march_raygen_rays_kernel.
// ---------------------------------------------------------------------------
// The 12 march words every record starts with.
__device__ __forceinline__ void store_march_words(uint32_t* rb, const Ray& nr) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ray_word(rb, kRayCen + i) = f2u(nr.cen[i]);
        ray_word(rb, kRayDir + i) = f2u(nr.dir[i]);
        ray_word(rb, kRayInvDir + i) = f2u(nr.invdir[i]);
    }
    ray_word(rb, kRayT) = f2u(nr.t);
    ray_word(rb, kRayTmax) = f2u(nr.tmax);
    ray_word(rb, kRayDeltaScale) = f2u(nr.delta_scale);
}

// Ray `id` = (workgroup, wave, lane) of a list, set up as the ray of a pixel is behind screen2worlddir's matrix
// product: dir = normalize3<FMA>(dirs[id]), cen = origins[id], then setup_ray_from as an offscreen frame
// without mesh depth.  Every lane of the workgroup calls (GW = waves per workgroup); returns whether the lane
// holds a ray of the list (id < n) -- ray.alive then says whether it enters the volume.
// A wave's 64 triples are 768 contiguous bytes of each array, 768-byte aligned: they are read as whole
// lines -- lane l takes floats l, 64 + l, 128 + l -- and turned into triples through LDS (as query_kernel
// turns its points; the stride-3 reads are free of bank conflicts).
template <int FMA, int GW>
__device__ __forceinline__ bool list_ray(const KParams& p, const RayList& rl, int lane, int wave, uint32_t& id,
                                         Ray& ray, float* vdir) {
    typedef __attribute__((address_space(1))) const float vr_gcfloat_t;
    __shared__ float tr[GW][2][3 * kWave];
    const int64_t first = ((int64_t)blockIdx.x * GW + wave) * kWave;  // the wave's first ray
    const int64_t left = rl.n - first;
    const int count = left <= 0 ? 0 : (left < kWave ? (int)left : kWave);
    vr_gcfloat_t* const so = (vr_gcfloat_t*)rl.origins + first * 3;
    vr_gcfloat_t* const sd = (vr_gcfloat_t*)rl.dirs + first * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int f = c * kWave + lane;
        if (f < count * 3) {  // (nothing is read behind the list's last float)
            tr[wave][0][f] = so[f];
            tr[wave][1][f] = sd[f];
        }
    }
    __syncthreads();
    id = (uint32_t)first + (uint32_t)lane;
    reset_ray(ray);
    if (lane >= count) return false;
    if (p.N <= 0) return true;  // enable_draw = tree.N > 0
    float cen[3], dir[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        cen[c] = tr[wave][0][lane * 3 + c];
        dir[c] = tr[wave][1][lane * 3 + c];
    }
    normalize3<FMA>(dir);
    setup_ray_from<FMA>(p, cen, dir, ray, vdir, []() -> float { return 1e9f; });
    return true;
}

}  // namespace

}  // namespace vr
