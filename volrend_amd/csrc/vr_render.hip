// vr_render.hip -- gfx950 (CDNA4) PlenOctree ray-march kernels.
//
// Replaces the reference's device path: device::render_kernel
// (src/cuda/volrend.cu:78-173) with trace_ray (include/volrend/cuda/rt_core.cuh:66-196),
// query_single_from_root (include/volrend/internal/n3tree_query.hpp:13-48) and
// maybe_precalc_basis (include/volrend/internal/lumisphere.hpp:9-87) -- written
// from the algorithm, not from the CUDA text: wave64 8x8 pixel tiles, a device
// re-layout built at upload (sigma packed into the node words, padded 16-byte
// aligned SH records, a top grid + bricks lookup structure), integer digit descent for N=2
// (bit-identical to the float descent, see query_n2), march / shade phases,
// deterministic expf, explicit FP contraction policy.
//
// Built with -ffp-contract=off; see vr_device_math.h.
//
// This file: the kernels of a launch (ray generation, the persistent render kernel, the frame-table
// write, the probe) and their launchers.  Layout, colour, point query and rays: vr_dev_*.h; the
// upload-time build kernels: vr_tree_kernels.hip.
// The two big kernels (render_kernel, raygen_kernel) are templates with a trailing pack PLANES: empty for
// the colour flavours, <AovParams> for the flavours of vr_render_aov, which take the planes as one more
// kernel argument.  Per flavour the machine code is what two separate kernels would have
// (tools/kernel_digest.py, profiles/render_pair_template_digest.txt).
#include "vr_device_math.h"
#include "vr_internal.h"
#include "vr_dev_layout.h"
#include "vr_dev_shade.h"
#include "vr_dev_query.h"
#include "vr_dev_rays.h"
#include "vr_dev_march.h"

namespace vr {

namespace {

// Register budget of the fused FAST flavours, waves per SIMD (each measured; EXPERIMENTS.md):
constexpr int kSh16Waves = 5;   // 96 VGPRs (6 needs <= 80 and spills: 0.44 ms per C1 frame)
constexpr int kSh25Waves = 4;   // 128 VGPRs (5 = 96 VGPRs + 64 B of scratch with fenced shade math: 30 % slower)
constexpr int kSh9Waves = 7;    // 72 VGPRs without scratch since the lane's ray id lives in LDS and the round
                                // counters in scalar registers (round 5; C3 -1...-3 % against 6)
constexpr int kSh16Rows = 64;   // SH16 items per shade round (56 fits 24 waves per CU into the LDS, but measured
                                // slower: 0.275 against 0.265 ms per C1 frame)

// ---------------------------------------------------------------------------
// render_kernel: render_kernel + trace_ray of the reference
// (volrend.cu:78-173, rt_core.cuh:66-196) as a PERSISTENT wave64 kernel.
//
//   * The launch covers one or more frames of the same size (a batch of poses).  Ray
//     generation is a kernel of its own (raygen_kernel below: one lane per pixel at full
//     occupancy, FP64-heavy); the rays that enter the volume sit compacted in the ray buffer,
//     ray id -> (frame, 8x8 pixel block, pixel) by locate().
//   * A fixed number of waves (one 64-thread workgroup each) stays resident.  A wave owns a
//     chunk of consecutive ray ids (one atomic add on a queue head per chunk); whenever
//     >= refill_min lanes are idle, the k-th idle lane loads ray chunk_next + k from the
//     buffer.  Terminated rays are replaced in place -- live rays never move between lanes.
//   * The colour of a sample never feeds back into the march (only the
//     attenuation does), so colour evaluation is decoupled from the ray that
//     produced it.  The wave alternates two phases, each with most lanes busy:
//       march : descent + sigma test + attenuation / light update / stop test;
//               samples with sigma > sigma_thresh append a (leaf, weight, owner)
//               item to a wave-level LDS ring (ballot + mbcnt compaction);
//       shade : as soon as 64 items wait, every lane takes ONE item -- whoever
//               owns it -- the SH records arrive by LDS-DMA, the owner's basis through
//               ds_bpermute; then each owner adds the results
//               of its own items, oldest first (the reference's order per ray).
//   * Finished rays composite over the background, quantise and store their
//     pixel -- retired and refilled in batches of >= refill_min lanes, one memory round
//     trip per batch.
// Per-ray arithmetic and its order are exactly the reference's.
// ---------------------------------------------------------------------------
// Wave-private LDS of the march kernel (one wave per workgroup):
//   ring  : colour work items (leaf, weight, owner lane) in sample order
//   stage : the SH records of one shade round, DMA'd straight from HBM (global_load_lds)
//   res   : the three colour contributions of each item of the round (aliases the first
//           768 bytes of `stage`: every row has been consumed by then)
// The basis of a lane's ray lives in that lane's registers; the lane that shades one of its
// items reads it through the LDS crossbar (ds_bpermute).
// ---------------------------------------------------------------------------
constexpr int kRing = 128;   // capacity; at most 127 items are ever outstanding

// Record fetch of a shade round: a record of V 16-byte chunks is fetched by V adjacent lanes
// (one or two cache lines per group instead of one line per lane and chunk) with LDS-DMA loads:
// lane l of an instruction lands at base + 16*l, i.e. records sit in dense rows of V*16 bytes
// and nothing passes through registers.  All records of a round (SH25: of half a round) are in
// flight at once; one wait, then every lane reads the row of the item it shades.
template <int BASIS>
struct Stage {
    static constexpr bool kEnabled = BASIS > 1;
    static constexpr int kVec = kEnabled ? RecTraits<BASIS>::kDwords / 4 : 1;  // V: 2, 4, 6, 10
    static constexpr int kRow = kVec * 16;                            // bytes
    static constexpr int kPerInstr = kWave / kVec;                    // records per DMA instruction
    // Rows per pass: SH16 (96-byte rows) shades kSh16Rows = 64 items per round in one pass
    // (6 KB of rows), SH25 (160-byte rows) 64 items in two passes of 32, the narrower formats 64
    // items in one pass.
    static constexpr int kPass = !kEnabled ? kWave
                                 : (kRow * kWave <= 5504 ? kWave
                                    : (BASIS == BASIS_16 ? kSh16Rows : kWave / 2));  // rows per pass
    static constexpr int kPasses = (BASIS == BASIS_25) ? 2 : 1;
    static constexpr int kShade = kPass * kPasses;                    // items per shade round
    static constexpr int kInstr = (kPass + kPerInstr - 1) / kPerInstr;
    static constexpr int kBytes = (kEnabled && kPass * kRow > 768) ? kPass * kRow : 768;
};
typedef __attribute__((address_space(1))) const void* vr_gptr_t;
typedef __attribute__((address_space(3))) void* vr_lptr_t;
// Outstanding colour items per ray: four 8-bit ring positions packed in one register, the newest
// in the top byte (a push is ONE v_alignbit_b32), the oldest at bit `qsh` = 32 - 8 * count (a pop
// only moves qsh).  (Eight per ray, measured: -2 % on a lone 20-frame launch, nothing on a
// 64-frame one, for a second register and a 64-bit funnel shift per push.)
constexpr int kOwnerQ = 4;

// The record requests of one pass of a shade round (see Stage): lane l fetches 16-byte chunk
// l % V of record l / V of its instruction, straight into the stage rows.  NT = the non-temporal
// cache policy (an immediate of the instruction, hence a template parameter).
template <int BASIS, bool NT, int RING = kRing>
__device__ __forceinline__ void issue_records(const KParams& p, char* stage, const uint32_t* it_leaf,
                                              uint32_t ring_head, int lane, int n, int pass) {
    using ST = Stage<BASIS>;
#pragma unroll
    for (int k = 0; k < ST::kInstr; ++k) {
        const int rin = k * ST::kPerInstr + lane / ST::kVec;  // record within the pass
        const int item = pass * ST::kPass + rin;
        if (lane < ST::kPerInstr * ST::kVec && rin < ST::kPass && item < n) {
            const uint32_t leaf = it_leaf[(ring_head + (uint32_t)item) & (RING - 1)];
            const char* src = reinterpret_cast<const char*>(p.leaves) +
                              (uint64_t)leaf * (uint32_t)(p.leaf_stride_h * 2) + (lane % ST::kVec) * 16;
            // (the LDS address is formed in address space 3: a generic-pointer detour between two
            // casts does not fold when `stage` is not the first LDS object of the kernel)
            __builtin_amdgcn_global_load_lds(
                (vr_gptr_t)src,
                (vr_lptr_t)((__attribute__((address_space(3))) char*)stage + k * ST::kPerInstr * ST::kRow),
                16, 0, NT ? 2 /* nt */ : 0);
        }
    }
}

// Waves per SIMD a flavour is compiled for: the fused FAST flavours their budgets above (SH25
// gathers its 25 basis values up front), the small records 8.  The instrumented / lobe / generic
// flavours keep their wider state in registers at 4 waves per SIMD (3 for SH25).  No render
// flavour uses scratch.
template <int BASIS, int MODE>
constexpr int min_waves_per_eu() {
    if (MODE != MODE_FAST) return BASIS == BASIS_25 ? 3 : 4;  // SH25 + counters needs > 128 VGPRs
    return BASIS == BASIS_25 ? kSh25Waves : BASIS == BASIS_16 ? kSh16Waves : BASIS == BASIS_9 ? kSh9Waves : 8;
}
// Waves one CU holds of a flavour: the register bound above or the LDS bound (512-byte granules).
// The AOV flavours of SH9 / SH16 / SH25 sit on their register steps (one more live register spills in
// the FMA SH9 flavour and costs the other two a wave): they keep the depth sum in one more LDS word per lane.
template <int BASIS, int MODE>
constexpr bool aov_depth_in_lds() {
    return MODE == MODE_FAST && (BASIS == BASIS_9 || BASIS == BASIS_16 || BASIS == BASIS_25);
}
template <int BASIS, int MODE, bool AOV = false>
constexpr int waves_per_cu() {
    const int lds = ((kRing * 9 + kWave * 4 + (AOV && aov_depth_in_lds<BASIS, MODE>() ? kWave * 4 : 0) +
                      Stage<BASIS>::kBytes + 511) / 512) * 512;
    const int by_lds = 163840 / lds, by_reg = 4 * min_waves_per_eu<BASIS, MODE>();
    return by_lds < by_reg ? by_lds : by_reg;
}

// The planes of one retired ray (vr_render_aov), always in frame position: D (times delta_scale for
// VR_DEPTH_WORLD, formed by the caller) and the transmittance the ray left the loop with.
__device__ __forceinline__ void store_aov(const AovParams& a, int frame, uint32_t xy, float d, float tr) {
    const AovDesc pl = a.planes[frame];
    const int64_t off = (int64_t)(xy >> 16) * a.pitch + (int64_t)(xy & 0xFFFFu) * 4;
    typedef __attribute__((address_space(1))) float vr_gfloat_t;
    if (pl.depth) *(vr_gfloat_t*)(reinterpret_cast<char*>(pl.depth) + off) = d;
    if (pl.transmittance) *(vr_gfloat_t*)(reinterpret_cast<char*>(pl.transmittance) + off) = tr;
}

// The record of a colour ray (vr_internal.h kRay*), into ray slot `slot`: what raygen_rays_kernel appends for a
// ray that enters the volume -- the tail of raygen_kernel, word for word.  (raygen_kernel keeps its own copy:
// calling this function from it changes the machine code of the frame kernels, tools/kernel_digest.py.)
template <int FMA, bool FULL>
__device__ __forceinline__ void store_colour_ray(const KParams& p, uint32_t slot, const Ray& nr, uint32_t xy,
                                                 uint8_t* px, int frame, const float* vdir) {
    uint32_t* rb = ray_slot(p.ray_buf_rw, kRayWords + p.ray_tail_words, slot);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ray_word(rb, kRayCen + i) = f2u(nr.cen[i]);
        ray_word(rb, kRayDir + i) = f2u(nr.dir[i]);
        ray_word(rb, kRayInvDir + i) = f2u(nr.invdir[i]);
    }
    ray_word(rb, kRayT) = f2u(nr.t);
    ray_word(rb, kRayTmax) = f2u(nr.tmax);
    ray_word(rb, kRayDeltaScale) = f2u(nr.delta_scale);
    ray_word(rb, kRayXy) = xy;
    ray_word(rb, kRayPixelLo) = (uint32_t)reinterpret_cast<uint64_t>(px);
    ray_word(rb, kRayPixelHi) = (uint32_t)(reinterpret_cast<uint64_t>(px) >> 32);
    ray_word(rb, kRayFrame) = (uint32_t)frame;
    if (p.ray_vdir) {
        // SH trees: the (rotated) view direction travels, its basis is evaluated when a lane takes
        // the ray (3 words instead of up to 25: the ray buffer is written and read once per ray)
#pragma unroll
        for (int i = 0; i < 3; ++i) ray_word(rb, kRayTail + i) = f2u(vdir[i]);
    } else if (p.basis_words > 0) {
        // rt_core.cuh:96-103: basis of the view direction, zeroed outside basis_minmax
        float b[VR_MAX_BASIS];
#pragma unroll
        for (int i = 0; i < VR_MAX_BASIS; ++i) b[i] = 0.f;
        precalc_basis<FMA, FULL>(p, vdir, b);
#pragma unroll
        for (int i = 0; i < VR_MAX_BASIS; ++i)
            if (i < p.basis_words)
                ray_word(rb, kRayTail + i) = f2u((i < p.basis_min || i > p.basis_max) ? 0.f : b[i]);
    }
}

// The planes of a kernel's pack PLANES: the AOV flavours' argument, or an empty table that the colour flavours
// never read.
__device__ __forceinline__ AovParams aov_arg() { return AovParams{}; }
__device__ __forceinline__ const AovParams& aov_arg(const AovParams& a) { return a; }

template <int FMA, int BASIS, int MODE, bool BLK, typename... PLANES>
__global__ __launch_bounds__(kWave, (min_waves_per_eu<BASIS, MODE>()))
void render_kernel(const KParams p, const PLANES... planes) {
    constexpr bool AOV = sizeof...(PLANES) != 0;
    const AovParams aov = aov_arg(planes...);
    using P = Policy<FMA>;
    constexpr bool N2 = MODE != MODE_GENERIC;
    constexpr bool LOBES = MODE != MODE_FAST;
    constexpr bool COUNT = MODE != MODE_FAST;
    constexpr int NB = BASIS > 1 ? BASIS : 1;
    constexpr bool HAS_BASIS = BASIS != BASIS_RGBA;
    using ST = Stage<BASIS>;
    __shared__ uint32_t it_leaf[kRing];
    __shared__ float it_w[kRing];
    __shared__ uint8_t it_own[kRing];
    __shared__ __attribute__((aligned(16))) char stage[ST::kBytes];
    float* const res = reinterpret_cast<float*>(stage);  // 3 x 64 floats, see above
    float mybasis[NB];  // basis_fn of this lane's ray (rt_core.cuh:96-103), read by shader lanes
#pragma unroll
    for (int i = 0; i < NB; ++i) mybasis[i] = 0.f;

    const int lane = threadIdx.x & (kWave - 1);
    Ray ray;
    ray.active = false;
    ray.alive = ray.entered = ray.stopped = false;
    // index of the lane's ray in the ray buffer: written when the lane takes the ray, read when it
    // retires it -- in LDS, not in a register that would sit idle through every march round
    __shared__ uint32_t ray_ids[kWave];
    ray.t = 0.f;
    ray.tmax = -1.f;
    ray.light = 1.f;
    ray.delta_scale = 1.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ray.cen[i] = 0.f;
        ray.dir[i] = 0.f;
        ray.invdir[i] = 1.f;
    }
    ray.out[0] = ray.out[1] = ray.out[2] = ray.out[3] = 0.f;
    RayCounters rc;
    Cursor cur;
    uint32_t qpos = 0;  // ring positions of this ray's outstanding items, see kOwnerQ
    uint32_t qsh = 32;  // 32 - 8 * (number of outstanding items)
    uint32_t rounds = 0, progress_round = 0;  // march rounds of this wave; the last one before a retire
    // wave-uniform scheduler state
    bool exhausted = false;  // the ray buffer has been handed out completely
    uint32_t chunk_next = 0, chunk_end = 0;  // this wave's private range of ray ids
    uint32_t ring_head = 0, ring_tail = 0;  // items [head, tail) are waiting for a shader lane
    const int wpr = kRayWords + p.ray_tail_words;  // words per ray in the ray buffer
    // scheduling statistics (instrumented flavours only): rounds and busy lanes per phase
    uint32_t st_march_r = 0, st_march_l = 0, st_shade_r = 0, st_shade_l = 0, st_distinct = 0,
             st_fin_r = 0, st_fin_l = 0, st_iter = 0;
    // AOV flavours: D of the lane's ray -- a register where the flavour has one to spare, else a
    // per-lane LDS word (read, multiply-add, write per hit sample: the rounding of either FP model)
    constexpr bool D_LDS = AOV && aov_depth_in_lds<BASIS, MODE>();
    float d_reg = 0.f;
    float* d_lds = nullptr;
    if constexpr (D_LDS) {
        __shared__ float d_words[kWave];
        d_lds = d_words;
    }
    auto depth_get = [&]() -> float {
        if constexpr (D_LDS) return d_lds[lane_id_now()];
        else return d_reg;
    };
    auto depth_set = [&](float v) {
        if constexpr (D_LDS) d_lds[lane_id_now()] = v;
        else d_reg = v;
    };

    // Colour evaluation of up to 64 queued items, one per lane, whoever owns them;
    // afterwards every owner adds the contributions of its own items, oldest first
    // (= the reference's accumulation order, rt_core.cuh:161).
    auto shade_chunk = [&](int n) {
        __syncthreads();  // item pushes are visible
        if (COUNT) {
            st_shade_r++;
            st_shade_l += (uint32_t)n;
            // distinct leaves among the chunk's items (instrumentation only)
            const uint32_t myleaf =
                lane < n ? it_leaf[(ring_head + (uint32_t)lane) & (kRing - 1)] : 0xFFFFFFFFu;
            bool first = lane < n;
            for (int o = 0; o < kWave; ++o) {
                const uint32_t other = (uint32_t)__shfl((int)myleaf, o);
                if (o < lane && other == myleaf) first = false;
            }
            st_distinct += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(first));
            if (lane < n)  // the record this item reads (colour coefficients only: sigma rides in the node word)
                touch(p, TOUCH_LEAVES, (uint64_t)myleaf * (uint32_t)(p.leaf_stride_h * 2),
                      (uint32_t)(2 * (p.data_dim - 1)));
        }
        const bool have = lane < n;
        const uint32_t jmine = (ring_head + (uint32_t)lane) & (kRing - 1);
        const float weight = have ? it_w[jmine] : 0.f;
        // basis_fn[i] of the ray that owns my item, out of its lane's registers through the LDS
        // crossbar (every lane executes the permute: a bpermute only reads active lanes)
        const int own4 = (HAS_BASIS && have) ? (int)it_own[jmine] << 2 : lane << 2;
        auto basis_of = [&](int i) -> float {
            return u2f((uint32_t)__builtin_amdgcn_ds_bpermute(own4, (int)f2u(mybasis[i])));
        };
        // One-pass flavours fetch each group of basis values one group ahead of where the (whole) wave
        // uses it (SumsAhead); the two-pass flavour (SH25) computes with half the wave at a time, so it
        // gathers everything up front while every owner lane is still active.
        float bfull[ST::kPasses > 1 ? NB : 1];
        if constexpr (ST::kPasses > 1) {
#pragma unroll
            for (int i = 0; i < NB; ++i) bfull[i] = basis_of(i);
        }
        auto basis_get = [&](int i) -> float {
            if constexpr (ST::kPasses > 1) return bfull[i];
            else return basis_of(i);
        };
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
        if constexpr (ST::kEnabled) {
#pragma unroll
            for (int pass = 0; pass < ST::kPasses; ++pass) {
                if (pass * ST::kPass < n) {  // wave-uniform
                    // Cache policy of the record stream (launch-uniform, chosen at upload): by
                    // default the records allocate in L2 like any load -- neighbouring rays
                    // re-use a quarter of them; when the lookup structure is much larger than
                    // the L2s, the stream is marked non-temporal so that it stops evicting the
                    // top / brick lines every sample needs (C3: -11 % time; C1-class trees:
                    // +8 %, hence the switch).  The policy is an immediate of the instruction,
                    // so the issue loop exists twice.
                    if (p.records_nt)
                        issue_records<BASIS, true>(p, stage, it_leaf, ring_head, lane, n, pass);
                    else
                        issue_records<BASIS, false>(p, stage, it_leaf, ring_head, lane, n, pass);
                    // (one pass: the owner's first basis values -- b0 and the first group, vr_dev_shade.h SumsAhead
                    // -- are requested here, in front of the wait: their LDS round trips run under the DMA's)
                    SumsAhead<FMA, ST::kPasses == 1 ? BASIS : 16> sums;
                    if constexpr (ST::kPasses == 1) sums.begin(basis_get);
                    __syncthreads();  // the DMAs have landed (vmcnt(0)) and are visible
                    // (one pass: ALL lanes run the arithmetic -- an owner lane without an item
                    // of its own must stay active for the permutes; only `have` lanes keep results)
                    if (ST::kPasses == 1 || lane / ST::kPass == pass) {
                        const char* row = stage + (lane % ST::kPass) * ST::kRow;
                        float acc[3];
                        if constexpr (ST::kPasses == 1) sums.finish(row, basis_get, acc);
                        else channel_sums<FMA, BASIS>(row, basis_get, acc);
                        // rt_core.cuh:161: weight / (1 + expf(-tmp)) per channel
                        // (the sigmoids of channels 0 / 1 share packed mul / fma / add instructions)
                        const float2v s01 = weighted_sigmoid2(weight, acc[0], acc[1]);
                        r0 = s01.x;
                        r1 = s01.y;
                        r2 = weighted_sigmoid(weight, acc[2]);
                    }
                    if (ST::kPasses > 1) __syncthreads();  // rows are free for the next pass
                }
            }
        } else {
          const float b0 = HAS_BASIS ? basis_of(0) : 0.f;  // (every lane: see above)
          if (have) {
            Record<BASIS> rec;
            load_record<BASIS>(p, it_leaf[jmine], rec);
            if (HAS_BASIS) {  // runtime basis size: first coefficient of each channel only
                r0 = weighted_sigmoid(weight, b0 * rec.at(0));
                r1 = weighted_sigmoid(weight, b0 * rec.at(1));
                r2 = weighted_sigmoid(weight, b0 * rec.at(2));
            } else {  // RGBA: out[c] = madd(colour, weight, out[c]) is formed by the owner
                r0 = rec.at(0);
                r1 = rec.at(1);
                r2 = rec.at(2);
            }
          }
        }
        __syncthreads();  // every row has been read: `res` may overwrite them
        if (have) {
            res[0 * kWave + lane] = r0;
            res[1 * kWave + lane] = r1;
            res[2 * kWave + lane] = r2;
        }
        __syncthreads();  // contributions are visible
        const uint32_t head8 = ring_head & 0xFFu;
#pragma unroll
        for (int d = 0; d < kOwnerQ; ++d) {
            const uint32_t pos = __builtin_amdgcn_ubfe(qpos, qsh, 8u);  // my oldest item
            const uint32_t idx = (pos - head8) & 0xFFu;               // its index within the round
            if (qsh < 32u && idx < (uint32_t)n) {
                if (HAS_BASIS) {
                    ray.out[0] += res[0 * kWave + idx];
                    ray.out[1] += res[1 * kWave + idx];
                    ray.out[2] += res[2 * kWave + idx];
                } else {
                    const float w = it_w[pos & (kRing - 1)];
                    ray.out[0] = P::madd(res[0 * kWave + idx], w, ray.out[0]);
                    ray.out[1] = P::madd(res[1 * kWave + idx], w, ray.out[1]);
                    ray.out[2] = P::madd(res[2 * kWave + idx], w, ray.out[2]);
                }
                qsh += 8u;
            }
        }
        ring_head += (uint32_t)n;
    };

    for (;;) {
        // ---- retire finished rays and hand their lanes new ones, in batches ----
        // A lane's ray is alive while t < tmax.  Nothing else says so: a ray that is cut short by
        // stop_thresh gets tmax = -1 (which finish_ray reads as "stopped"), a lane without a ray
        // has t = 0, tmax = -1.  (As loop-carried booleans the two cost the scalar unit -- shared
        // by the CU's four SIMDs -- about sixteen lane-mask copies and merges per march round.)
        const bool done = ray.active && !(ray.t < ray.tmax) && qsh == 32u;
        const unsigned long long m_done = __builtin_amdgcn_ballot_w64(done);
        const unsigned long long m_free = __builtin_amdgcn_ballot_w64(!ray.active);
        const unsigned long long m_busy =
            __builtin_amdgcn_ballot_w64(ray.active && (ray.t < ray.tmax || qsh < 32u));
        const int n_avail = __builtin_popcountll(m_done | m_free);
        if (COUNT) st_iter++;
        if (n_avail > 0 && (m_busy == 0ull || (!exhausted && n_avail >= p.refill_min))) {
            if (COUNT && m_done != 0ull) {
                st_fin_r++;
                st_fin_l += (uint32_t)__builtin_popcountll(m_done);
            }
            // The whole round costs ONE memory round trip: the pixel address of every finished
            // ray is requested here, the new rays right behind it, and the finished rays are
            // composited and stored once everything has landed (their colour state does not
            // overlap the registers the new rays load into).
            uint32_t px_lo = 0, px_hi = 0, fin_xy = 0, fin_frame = 0;
            float fin_d = 0.f;  // (AOV) the depth plane's value, formed before a new ray's delta_scale lands
            ray.stopped = ray.tmax < 0.f;  // (read before a new ray's tmax lands in the register)
            if (done) {
                const uint32_t* rs = ray_slot(p.ray_buf, wpr, ray_ids[lane_id_now()]);
                px_lo = ray_word(rs, kRayPixelLo);
                px_hi = ray_word(rs, kRayPixelHi);
                if (COUNT || p.any_accum || AOV) {
                    fin_xy = ray_word(rs, kRayXy);
                    fin_frame = ray_word(rs, kRayFrame);
                }
                if constexpr (AOV) {
                    fin_d = depth_get();
                    if (aov.depth_world) fin_d = fin_d * ray.delta_scale;
                }
            }
            const bool vacant = done || !ray.active;
            bool take = false;
            // (a ray retires in this pass: the wave makes progress.  A finished ray that still WAITS for a
            // pass -- fewer than refill_min idle lanes -- does not count: were it to, a wave that holds one
            // finished and one endless ray after the queues ran dry would never trip the guard.  Both
            // counters are wave-uniform; saying so keeps them in scalar registers -- as vector values they
            // cost the SH16 flavour its last two)
            if (m_done != 0ull) progress_round = (uint32_t)__builtin_amdgcn_readfirstlane((int)rounds);
            // Idle lanes take consecutive rays from the buffer.  The wave owns a private
            // chunk [chunk_next, chunk_end) of ray ids and only goes to the global queue
            // head (ONE returning atomic -- a single word sustains ~90 of them per
            // microsecond chip-wide) when the chunk is used up; chunk sizes shrink as the
            // queue drains (guided self-scheduling) so the tail stays balanced.
            if (!exhausted && chunk_next >= chunk_end) {
                uint32_t lo, hi;
                grab_chunk(p, lane, lo, hi);
                lo = __builtin_amdgcn_readfirstlane(lo);
                hi = __builtin_amdgcn_readfirstlane(hi);
                if (hi == lo) {
                    exhausted = true;
                } else {
                    chunk_next = lo;
                    chunk_end = hi;
                }
            }
            if (!exhausted) {
                const unsigned long long idle = m_done | m_free;
                const uint32_t r = chunk_next + lane_rank(idle);
                const uint32_t c_end = chunk_end;
                const uint32_t left = chunk_end - chunk_next;
                chunk_next += (uint32_t)n_avail < left ? (uint32_t)n_avail : left;
                if (vacant && r < c_end) {
                    take = true;
                    const uint32_t* rs = ray_slot(p.ray_buf, wpr, r);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        ray.cen[i] = u2f(ray_word(rs, kRayCen + i));
                        ray.dir[i] = u2f(ray_word(rs, kRayDir + i));
                        ray.invdir[i] = u2f(ray_word(rs, kRayInvDir + i));
                    }
                    ray.t = u2f(ray_word(rs, kRayT));
                    ray.tmax = u2f(ray_word(rs, kRayTmax));
                    ray.delta_scale = u2f(ray_word(rs, kRayDeltaScale));
                    ray_ids[lane_id_now()] = r;
                    if (HAS_BASIS) {
                        if (BASIS > 1 && p.ray_vdir) {
                            // rt_core.cuh:96-103: the basis of the ray's view direction (SH:
                            // lumisphere.hpp:38-81), zeroed outside basis_minmax -- evaluated
                            // here, by the lane that takes the ray, from 3 words of the record
                            float vd[3];
#pragma unroll
                            for (int i = 0; i < 3; ++i) vd[i] = u2f(ray_word(rs, kRayTail + i));
                            precalc_basis<FMA, false, (BASIS > 1 ? BASIS : 1)>(p, vd, mybasis);
#pragma unroll
                            for (int i = 0; i < NB; ++i)
                                if (i < p.basis_min || i > p.basis_max) mybasis[i] = 0.f;
                        } else {
#pragma unroll
                            for (int i = 0; i < NB; ++i)
                                mybasis[i] = u2f(ray_word(rs, kRayTail + i));
                        }
                    }
                }
            }
            if (done)
                finish_ray<FMA, COUNT>(
                    p, ray, rc,
                    reinterpret_cast<uint8_t*>(((uint64_t)px_hi << 32) | (uint64_t)px_lo), fin_xy,
                    (int)fin_frame);
            if constexpr (AOV) {
                if (done) store_aov(aov, (int)fin_frame, fin_xy, fin_d, ray.light);
                if (vacant) depth_set(0.f);
            }
            if (vacant) {
                ray.active = ray.entered = take;
                if (!take) {  // (no ray: not alive)
                    ray.t = 0.f;
                    ray.tmax = -1.f;
                }
                ray.out[0] = ray.out[1] = ray.out[2] = ray.out[3] = 0.f;
                ray.light = 1.f;
                rc = RayCounters();
                cur = Cursor();
                qsh = 32u;
                qpos = 0;
            }
        }
        if (!wave_any(ray.active)) {
            if (exhausted) break;
            continue;
        }

        // ---- march: lanes with a live ray and room for another outstanding item ----
        // Guard against rays that never end (not in the reference, which would spin): when the
        // wave has marched p.max_iter rounds (tuning key `max_iter`, for tests) since its last
        // retire / refill pass that retired a ray
        // (progress_round above: with the default of 2^22 rounds the difference to "without a
        // retired ray" is nil; a lowered max_iter trips earlier the larger refill_min is), whatever is still
        // marching is cut and reported (sticky status bit 0: the host layers fail loudly on it;
        // WHICH rays share a wave depends on the scheduling knobs, so the pixels of a launch that
        // tripped the guard are not tuning-independent -- they are wrong either way).  Wave-uniform
        // and checked once per pass through here (<= march_max rounds), so that a march round
        // carries nothing of it (five vector and four scalar instructions per round until round 3;
        // -2 % frame time, profiles/r04_*).
        if (rounds - progress_round >= (uint32_t)p.max_iter) {
            if (ray.t < ray.tmax) {
                ray.t = ray.tmax;
                if (p.status) atomicOr(p.status, 1u);
            }
            progress_round = rounds;
        }
        int m = 0;
        for (; m < p.march_max; ++m) {
            // (the wave's "anybody marching?" mask comes straight from the two compares: the
            // ballot of a combined boolean costs two more vector instructions)
            const unsigned long long m_go = __builtin_amdgcn_ballot_w64(ray.t < ray.tmax) &
                                            __builtin_amdgcn_ballot_w64(qsh != 0u);
            if (m_go == 0ull) break;
            const bool go = ray.t < ray.tmax && qsh != 0u;
            if (COUNT) {
                st_march_r++;
                st_march_l += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(go));
            }
            bool push = false;
            uint32_t leaf = 0;
            float weight = 0.f;
            if (go) {
                float pos[3];
                pos[0] = P::madd(ray.t, ray.dir[0], ray.cen[0]);
                pos[1] = P::madd(ray.t, ray.dir[1], ray.cen[1]);
                pos[2] = P::madd(ray.t, ray.dir[2], ray.cen[2]);
                float cube_sz = 0.f;
                int levels;
                uint32_t word;
                if (N2) {
                    leaf = query_n2<COUNT, (MODE == MODE_FAST ? (BLK ? 1 : 0) : -1)>(p, pos, &levels, &word, cur);
                } else {
                    leaf = (uint32_t)query_generic<FMA, COUNT>(p, pos, &cube_sz, &levels, &word);
                }
                if (COUNT) {
                    rc.samples++;
                    rc.child_reads += (uint32_t)levels;
                }
                // rt_core.cuh:116: dda / cube_sz
                const float dda = dda_unit<FMA>(pos, ray.invdir);
                // N2: cube_sz = 2^levels; x / 2^k == ldexp(x, -k), the same real number rounded once
                const float t_subcube =
                    N2 ? __builtin_amdgcn_ldexpf(dda, -levels) : dda / cube_sz;
                const float delta_t = t_subcube + p.step_size;
                const float sigma = h2f((uint16_t)(word & 0xFFFFu));
                bool stop = false;
                if (sigma > p.sigma_thresh) {
                    // rt_core.cuh:118-121,174: attenuation, weight and the light update are
                    // taken now; the colour of this sample -- which nothing else depends on --
                    // becomes a work item for the shade phase.
                    if (COUNT) rc.hits++;
                    // vr_expf_nonan: for a ray with a finite, non-zero direction the argument is not
                    // NaN -- sigma > sigma_thresh is false for a NaN sigma, delta_scale = 1 / |dir| is
                    // finite and positive, and delta_t is never NaN (dda_unit is a minimum with 1e4,
                    // which drops a NaN), so a sigma of +inf gives +-inf.  (Only a product
                    // delta_t * delta_scale that rounds to 0, below 2^-150, could meet an infinite sigma
                    // as 0 * inf.)  Every non-NaN argument, +-inf included, gives the bits of vr_expf
                    // (tests/test_gpu_device_forms.py sweeps them all); a NaN one -- a ray list may hand
                    // in a direction that is not finite -- gives 0 or +inf where vr_expf gives NaN.
                    const float att = vr_expf_nonan(-delta_t * ray.delta_scale * sigma);
                    weight = ray.light * (1.f - att);
                    if constexpr (AOV) depth_set(P::madd(weight, ray.t, depth_get()));
                    if (COUNT && p.render_depth)  // (depth launches take the FULL flavour)
                        ray.out[0] = P::madd(weight, ray.t, ray.out[0]);
                    else
                        push = true;
                    ray.light *= att;
                    stop = ray.light < p.stop_thresh;
                }
                if (stop) {
                    ray.tmax = -1.f;  // stopped (and no longer alive)
                    if (COUNT) rc.early++;
                } else {
                    ray.t += delta_t;
                }
            }
            // append this step's items to the ring: k-th pushing lane -> tail + k
            const unsigned long long m_push = __builtin_amdgcn_ballot_w64(push);
            if (m_push != 0ull) {
                if (push) {
                    const uint32_t seq = ring_tail + lane_rank(m_push);
                    const uint32_t j = seq & (kRing - 1);
                    it_leaf[j] = leaf;
                    it_w[j] = weight;
                    it_own[j] = (uint8_t)lane;
                    qpos = __builtin_amdgcn_alignbit(seq, qpos, 8u);  // (qpos >> 8) | seq << 24
                    qsh -= 8u;
                }
                ring_tail += (uint32_t)__builtin_popcountll(m_push);
                // (a loop: with rounds of fewer than 64 items -- kSh16Rows < 64 -- one round per
                // march step would let the ring overflow)
                while (ring_tail - ring_head >= (uint32_t)ST::kShade) shade_chunk(ST::kShade);
            }
            // Drain phase (the ray queues have run dry): a ray whose colour queue is full cannot
            // march until a shade round takes its items, and a round waits for 64 items or for the
            // moment NOBODY can march -- with few rays left in the wave the blocked ray waits for the
            // other rays to fill their queues too, i.e. the last rays of a launch take turns instead
            // of marching side by side (a one-frame launch ran 526 rounds in its longest-lived wave
            // for a longest ray of 230 samples; without colour work 279:
            // profiles/r05_tail_profile.jsonl).  So once the wave is down to drain_flush marching
            // lanes, a blocked ray gets a (partial) round at once.  (A partial round costs what a
            // full one costs: while the queues still feed the wave this would be a loss.)
            if (exhausted) {
                const unsigned long long m_alive = __builtin_amdgcn_ballot_w64(ray.t < ray.tmax);
                if (__builtin_popcountll(m_alive) <= p.drain_flush &&
                    (m_alive & __builtin_amdgcn_ballot_w64(qsh == 0u)) != 0ull && ring_tail != ring_head) {
                    const uint32_t waiting = ring_tail - ring_head;
                    shade_chunk(waiting < (uint32_t)ST::kShade ? (int)waiting : ST::kShade);
                }
            }
        }
        rounds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(rounds + (uint32_t)m));
        // nobody can march any more (queues full / rays ended): flush what is queued
        // (at most kShade - 1 + 64 items wait here: two rounds at most)
        while (ring_tail != ring_head && !wave_any(ray.t < ray.tmax && qsh > 0u)) {
            const uint32_t waiting = ring_tail - ring_head;
            shade_chunk(waiting < (uint32_t)ST::kShade ? (int)waiting : ST::kShade);
        }
    }
    if (COUNT && p.sched_stats && lane == 0) {
        atomicAdd(&p.sched_stats[kStatMarchRounds], (unsigned long long)st_march_r);
        atomicAdd(&p.sched_stats[kStatMarchLanes], (unsigned long long)st_march_l);
        atomicAdd(&p.sched_stats[kStatShadeRounds], (unsigned long long)st_shade_r);
        atomicAdd(&p.sched_stats[kStatShadeLanes], (unsigned long long)st_shade_l);
        atomicAdd(&p.sched_stats[kStatDistinctLeaves], (unsigned long long)st_distinct);
        atomicAdd(&p.sched_stats[kStatRetireRounds], (unsigned long long)st_fin_r);
        atomicAdd(&p.sched_stats[kStatRetiredRays], (unsigned long long)st_fin_l);
        atomicAdd(&p.sched_stats[kStatIterations], (unsigned long long)st_iter);
    }
}


// ---------------------------------------------------------------------------
// raygen_kernel: one lane per pixel of every frame of the launch, at full occupancy.
// Ray generation, NDC warp, world->tree transform, view-direction rotation and the
// ray/box test (volrend.cu:135-148, rt_core.cuh:74-92) with their FP64 islands,
// plus the basis of the view direction (rt_core.cuh:96-103).  Rays that miss the
// volume are composited and stored right here; the others are appended to the
// ray buffer -- each wave compacts its survivors with a ballot / mbcnt prefix
// count and reserves their slots with ONE atomic.
// ---------------------------------------------------------------------------
// Waves (8x8 pixel blocks) per raygen workgroup: 16, 4 or 1 (launch_render picks; tuning key
// raygen_waves).  16 for batches: one atomic per 1024 pixels.  Launches of one or two frames -- the
// ones whose neighbour on another stream is still draining -- use 4: a workgroup of 16 waves needs
// four free wave slots AND 256 free vector registers on every SIMD of one CU at the same moment,
// which the previous launch's render kernel (5 waves x 96 registers per SIMD) does not offer until
// it is nearly done: the ray generation of launch k + 1 took 135 us instead of 16 beside the tail
// of launch k (kernel trace, profiles/r06_overlap_trace.jsonl), 51 with workgroups of 4 -- and the
// render kernel of launch k + 1 cannot start before it has ended.  Smaller workgroups mean more
// atomics: at 4 waves a 64-frame launch is 4 % slower, at 1 wave 35 % (profiles/r06_raygen_waves.jsonl).

// (PLANES sits between two arguments and is never deduced: every use names it.)
// HEAD: the flavours with the lead-in march (vr_internal.h; FAST only).  It is a flavour and not a branch on
// HeadParams: with the loop in the kernel, ray generation without a lead-in takes 840 us instead of 567 us per
// 64-frame C1 launch (EXPERIMENTS.md "Lead-in march").  The flavours without it never read `head`.
template <int FMA, bool FULL, int GW, bool HEAD, typename... PLANES>
__global__ __launch_bounds__(kWave* GW)
void raygen_kernel(const KParams p, const PLANES... planes, const CullParams cull, const HeadParams head) {
    static_assert(!(HEAD && FULL), "the FULL flavours count every sample in the march kernel");
    constexpr bool AOV = sizeof...(PLANES) != 0;
    const AovParams aov = aov_arg(planes...);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const uint32_t id =
        (uint32_t)(((int64_t)blockIdx.x * GW + wave) * kWave + lane);
    bool valid = false;
    // Block cull (vr_internal.h; FAST flavours, cull.mask != NULL): the 64 lanes of a wave hold the pixels of ONE
    // 8x8 block of one frame.  When the block's bit of the launch's mask is clear, no ray of the block meets a
    // cell with density: all of them take the path of a ray that misses the volume, which leaves the same pixel.
    bool culled = false;
    Ray nr;
    uint8_t* px = nullptr;
    uint32_t xy = 0;
    int frame = 0;
    float vdir[3] = {0.f, 0.f, 1.f};
    // The lane's ray is set up: it goes to the ray buffer, or it is composited and stored right here.
    auto keep_or_finish = [&]() {
        if (nr.alive) {
            valid = true;
        } else {
            RayCounters z;  // a ray without a single sample (HEAD: or without one that is a hit)
            finish_ray<FMA, FULL>(p, nr, z, px, xy, frame);
            if constexpr (AOV) store_aov(aov, frame, xy, 0.f, 1.f);  // no hit sample: D = 0, T = 1
        }
    };
    bool has = false;  // (HEAD) the lane holds a pixel of the image
    if constexpr (HEAD) nr.alive = false;
    if (id < p.total_rays) {
        const PixelRef r = locate(p, id);
        if constexpr (!FULL) {
            if (cull.mask) {
                const uint32_t b = (uint32_t)(r.y >> 3) * cull.nbx + (uint32_t)(r.x >> 3);
                const uint32_t w = cull.mask[(size_t)r.frame * cull.words_per_frame + (b >> 5)];
                culled = __builtin_amdgcn_readfirstlane((int)((w >> (b & 31u)) & 1u)) == 0;  // (wave-uniform)
            }
        }
        if (r.in_image) {
            frame = r.frame;
            xy = (uint32_t)r.x | ((uint32_t)r.y << 16);
            px = pixel_ptr(p, p.frames[r.frame], r);
            if (culled) reset_ray(nr);
            else setup_ray<FMA>(p, r, nr, vdir);
            if constexpr (HEAD) has = true;
            else keep_or_finish();
        }
    }
    // Lead-in march: the block's rays step through the empty space in front of their first hit sample here, side
    // by side (every lane of the wave is here); a ray that ends there is no longer alive and takes the path of a
    // ray without a sample -- finish_ray reads entered = true, light = 1: alpha = 0.
    uint32_t head_n[kHeadStatWords] = {0u, 0u, 0u};  // (wave-uniform) rays entered, retired, samples marched
    if constexpr (HEAD) {
        head_n[0] = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(nr.alive));
        if (head_n[0] != 0u)
            head_n[2] = p.brick_blocked ? head_march<FMA, kQueryN2Blocked>(p, head, nr)
                                        : head_march<FMA, kQueryN2>(p, head, nr);
        head_n[1] = head_n[0] - (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(nr.alive));
        if (has) keep_or_finish();
    }
    // compaction into the queue that owns the workgroup's blocks (vr_dev_rays.h)
    const unsigned long long m_valid = __builtin_amdgcn_ballot_w64(valid);
    __shared__ uint32_t wave_culled[GW];  // (read behind the barriers of reserve_ray_slots)
    __shared__ uint32_t wave_head[HEAD ? GW : 1][kHeadStatWords];
    if constexpr (!FULL && GW > 1) {
        if (cull.mask && lane == 0) wave_culled[wave] = culled ? 1u : 0u;
        if constexpr (HEAD) {
            if (lane < kHeadStatWords) wave_head[wave][lane] = lane == 0 ? head_n[0] : lane == 1 ? head_n[1] : head_n[2];
        }
    }
    const uint32_t my_base = reserve_ray_slots<GW>(p, m_valid, lane, wave);
    if constexpr (!FULL) {
        // the observable (vr_tree_cull_stats): blocks seen and blocks culled by this workgroup, one atomic
        // instruction (two lanes, two words of one line; the lines are dealt over the workgroups)
        if (cull.mask && threadIdx.x < 2u) {
            const int64_t left = (int64_t)(p.total_rays >> 6) - (int64_t)blockIdx.x * GW;
            uint32_t n = (uint32_t)(left < 0 ? 0 : (left < GW ? left : GW));
            if (threadIdx.x == 1u) {
                if constexpr (GW > 1) {
                    n = 0;
#pragma unroll
                    for (int w = 0; w < GW; ++w) n += wave_culled[w];
                } else {
                    n = culled ? 1u : 0u;
                }
            }
            if (n)
                atomicAdd(cull.stats + (blockIdx.x & (uint32_t)(kCullStatLines - 1)) * kCullStatStride + threadIdx.x,
                          (unsigned long long)n);
        }
    }
    if constexpr (HEAD) {
        // the observable (vr_tree_head_stats): the workgroup's three sums, one atomic instruction (three lanes,
        // three words of one line; the lines are dealt over the workgroups as the cull's are)
        if (threadIdx.x < (uint32_t)kHeadStatWords) {
            uint32_t n = 0;
            if constexpr (GW > 1) {
#pragma unroll
                for (int w = 0; w < GW; ++w) n += wave_head[w][threadIdx.x];
            } else {
                n = threadIdx.x == 0u ? head_n[0] : threadIdx.x == 1u ? head_n[1] : head_n[2];
            }
            if (n)
                atomicAdd(head.stats + (blockIdx.x & (uint32_t)(kCullStatLines - 1)) * kCullStatStride + threadIdx.x,
                          (unsigned long long)n);
        }
    }
    if (!valid) return;
    const uint32_t slot = my_base + lane_rank(m_valid);
    uint32_t* rb = ray_slot(p.ray_buf_rw, kRayWords + p.ray_tail_words, slot);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ray_word(rb, kRayCen + i) = f2u(nr.cen[i]);
        ray_word(rb, kRayDir + i) = f2u(nr.dir[i]);
        ray_word(rb, kRayInvDir + i) = f2u(nr.invdir[i]);
    }
    ray_word(rb, kRayT) = f2u(nr.t);
    ray_word(rb, kRayTmax) = f2u(nr.tmax);
    ray_word(rb, kRayDeltaScale) = f2u(nr.delta_scale);
    ray_word(rb, kRayXy) = xy;
    ray_word(rb, kRayPixelLo) = (uint32_t)reinterpret_cast<uint64_t>(px);
    ray_word(rb, kRayPixelHi) = (uint32_t)(reinterpret_cast<uint64_t>(px) >> 32);
    ray_word(rb, kRayFrame) = (uint32_t)frame;
    if (p.ray_vdir) {
        // SH trees: the (rotated) view direction travels, its basis is evaluated when a lane takes
        // the ray (3 words instead of up to 25: the ray buffer is written and read once per ray)
#pragma unroll
        for (int i = 0; i < 3; ++i) ray_word(rb, kRayTail + i) = f2u(vdir[i]);
    } else if (p.basis_words > 0) {
        // rt_core.cuh:96-103: basis of the view direction, zeroed outside basis_minmax
        float b[VR_MAX_BASIS];
#pragma unroll
        for (int i = 0; i < VR_MAX_BASIS; ++i) b[i] = 0.f;
        precalc_basis<FMA, FULL>(p, vdir, b);
#pragma unroll
        for (int i = 0; i < VR_MAX_BASIS; ++i)
            if (i < p.basis_words)
                ray_word(rb, kRayTail + i) = f2u((i < p.basis_min || i > p.basis_max) ? 0.f : b[i]);
    }
}

// ---------------------------------------------------------------------------
// raygen_rays_kernel: raygen_kernel for a ray list (vr_render_rays; vr_internal.h RayList): one lane per ray,
// 64 consecutive rays per wave in the caller's order.  The ray comes from list_ray() instead of locate() +
// setup_ray; its "pixel" is element `id` of the pseudo-frame's arrays.  A ray that misses the volume is
// composited and stored here, the others are compacted into the queues as raygen_kernel's records -- lanes
// behind the list's end neither reserve nor store.  (A list has no AOV planes.)
// ---------------------------------------------------------------------------
template <int FMA, bool FULL, int GW>
__global__ __launch_bounds__(kWave* GW) void raygen_rays_kernel(const KParams p, const RayList rl) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    uint32_t id;
    Ray nr;
    float vdir[3] = {0.f, 0.f, 1.f};
    const bool has = list_ray<FMA, GW>(p, rl, lane, wave, id, nr, vdir);
    bool valid = false;
    uint8_t* px = nullptr;
    uint32_t xy = 0;
    if (has) {
        xy = (id & (uint32_t)(kRayListWidth - 1)) | ((id >> kRayListShift) << 16);
        px = p.frames[0].rgba + (int64_t)id * 4;
        if (nr.alive) {
            valid = true;
        } else {
            RayCounters z;  // a ray without a single sample
            finish_ray<FMA, false>(p, nr, z, px, xy, 0);  // (COUNT: counters and depth mode, which a list never has)
        }
    }
    const unsigned long long m_valid = __builtin_amdgcn_ballot_w64(valid);
    const uint32_t my_base = reserve_ray_slots<GW>(p, m_valid, lane, wave);
    if (!valid) return;
    store_colour_ray<FMA, FULL>(p, my_base + lane_rank(m_valid), nr, xy, px, 0, vdir);
}

// Writes the per-launch frame table into device memory and resets the ray queue.
// (Stream-ordered replacement for a pinned-memory H2D copy + memset.)
// mask != NULL: also clears the block masks of its frames (words_per_frame, a multiple of 4, each) for
// block_mask_kernel.
__global__ void prepare_launch_kernel(FrameTable tbl, FrameDesc* frames, uint32_t* queue_head, uint32_t* mask,
                                      uint32_t words_per_frame) {
    const int i = threadIdx.x;
    if (i < tbl.n) frames[tbl.first + i] = tbl.f[i];
    if (tbl.first == 0 && i < kMaxQueues) {
        queue_head[i * kQueueStride + kQueueHead] = 0u;
        queue_head[i * kQueueStride + kQueueCount] = 0u;
    }
    if (mask) {
        uint4* const q = reinterpret_cast<uint4*>(mask + (size_t)tbl.first * words_per_frame);
        const uint32_t n = (uint32_t)tbl.n * (words_per_frame >> 2);
        for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) q[j] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// ---------------------------------------------------------------------------
// block_mask_kernel: the block masks of a launch (vr_internal.h "Block cull").  Workgroup (x, f) takes the x-th
// part of the tree's boundary-cell list for frame f: every cell is projected as its bounding sphere, the blocks
// the projection can touch are marked in an LDS copy of the frame's mask, and the copy's non-zero words are ORed
// into the mask of the launch slot.
//   Cell centre c (tree space) -> world (c - offset) / scale -> camera (X, Y, depth) by the frame's pose; the
//   sphere has the half-diagonal r of the cell's box in world space.  A point of the sphere, (X + a, Y + b,
//   depth + e) with a^2 + b^2 + e^2 <= r^2, lies on the ray of pixel x = w/2 + fx (X + a) / (depth + e), and
//   |(X + a) / (depth + e) - X / depth| = |a depth - X e| / (depth (depth + e)) <= r sqrt(depth^2 + X^2) /
//   (depth (depth - r)); likewise for y.  That half-width, times 1.05 plus one pixel for the rounding of ray
//   generation and of this kernel, gives the rectangle of pixels whose blocks are marked.
//   The whole frame is marked when a sphere comes within r / 100 of the camera plane (depth - r <= r / 100), when the
//   pose is not a rotation (to 1e-4) or anything here is not finite: such a frame is not culled.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void block_mask_kernel(const KParams p, const MaskParams m) {
    __shared__ uint32_t bits[kMaskMaxWords];
    __shared__ uint32_t whole;
    const uint32_t wpf = m.words_per_frame;
    for (uint32_t i = threadIdx.x; i < wpf; i += blockDim.x) bits[i] = 0u;
    if (threadIdx.x == 0) whole = 0u;
    __syncthreads();
    const int frame = blockIdx.y;
    const int g = m.levels;
    const uint32_t count = m.occ[0];
    const uint32_t* const list = m.occ + kOccHeaderWords + occ_bitmap_words(g);
    const uint32_t per = (count + (uint32_t)m.groups_per_frame - 1u) / (uint32_t)m.groups_per_frame;
    const uint32_t lo = blockIdx.x * per;
    const uint32_t hi = lo + per < count ? lo + per : count;
    float xf[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) xf[i] = p.frames[frame].xf[i];
    const float cell = u2f((uint32_t)(127 - g) << 23);  // 2^-g
    float inv_scale[3], r2 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        inv_scale[i] = 1.f / p.scale[i];
        const float h = 0.5f * cell * inv_scale[i];
        r2 += h * h;
    }
    const float r = __builtin_sqrtf(r2) * 1.0001f;
    // the pose must be a rotation for the sphere to stay one in camera space
    bool ok = r > 0.f && r < 1e30f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            const float d = xf[3 * a] * xf[3 * b] + xf[3 * a + 1] * xf[3 * b + 1] + xf[3 * a + 2] * xf[3 * b + 2];
            if (!(__builtin_fabsf(d - (a == b ? 1.f : 0.f)) <= 1e-4f)) ok = false;
        }
    const float afx = __builtin_fabsf(p.fx), afy = __builtin_fabsf(p.fy);
    const uint32_t n_mask = (1u << g) - 1u;
    const float fnbx = (float)m.nbx, fnby = (float)m.nby;
    if (!ok && lo < hi) whole = 1u;
    for (uint32_t idx = lo + threadIdx.x; ok && idx < hi; idx += blockDim.x) {
        const uint32_t c = list[idx];
        const float tc[3] = {((float)((c >> (2 * g)) & n_mask) + 0.5f) * cell, ((float)((c >> g) & n_mask) + 0.5f) * cell,
                             ((float)(c & n_mask) + 0.5f) * cell};
        float d[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = (tc[i] - p.offset[i]) * inv_scale[i] - xf[9 + i];
        const float X = xf[0] * d[0] + xf[1] * d[1] + xf[2] * d[2];
        const float Y = xf[3] * d[0] + xf[4] * d[1] + xf[5] * d[2];
        const float depth = -(xf[6] * d[0] + xf[7] * d[1] + xf[8] * d[2]);
        if (!(depth - r > 0.01f * r)) {
            // in front of the camera plane or through it -- or behind it: then no ray of the frame reaches the cell
            if (!(depth + r < 0.f)) whole = 1u;
            continue;
        }
        const float inv = 1.f / (depth * (depth - r));
        const float rx = afx * r * __builtin_sqrtf(depth * depth + X * X) * inv * 1.05f + 1.f;
        const float ry = afy * r * __builtin_sqrtf(depth * depth + Y * Y) * inv * 1.05f + 1.f;
        const float px = 0.5f * (float)p.width + p.fx * X / depth;
        const float py = 0.5f * (float)p.height - p.fy * Y / depth;
        // blocks [bx0, bx1] x [by0, by1], clamped in float (a NaN takes the whole row / column)
        const float fx0 = __builtin_floorf(__builtin_fmaxf((px - rx) * 0.125f, 0.f));
        const float fx1 = __builtin_floorf(__builtin_fminf((px + rx) * 0.125f, fnbx - 1.f));
        const float fy0 = __builtin_floorf(__builtin_fmaxf((py - ry) * 0.125f, 0.f));
        const float fy1 = __builtin_floorf(__builtin_fminf((py + ry) * 0.125f, fnby - 1.f));
        if (!(fx0 <= fx1) || !(fy0 <= fy1)) continue;  // beside the frame
        const uint32_t bx0 = (uint32_t)fx0, bx1 = (uint32_t)fx1, by0 = (uint32_t)fy0, by1 = (uint32_t)fy1;
        for (uint32_t by = by0; by <= by1; ++by) {
            const uint32_t first = by * m.nbx + bx0, last = by * m.nbx + bx1;
            for (uint32_t w = first >> 5; w <= (last >> 5); ++w) {
                const uint32_t from = w == (first >> 5) ? (first & 31u) : 0u;
                const uint32_t to = w == (last >> 5) ? (last & 31u) : 31u;
                const uint32_t mask = (0xFFFFFFFFu >> (31u - to)) & (0xFFFFFFFFu << from);
                if ((bits[w] & mask) != mask) atomicOr(&bits[w], mask);
            }
        }
    }
    __syncthreads();
    uint32_t* const out = m.mask + (size_t)frame * wpf;
    const bool all = whole != 0u;
    for (uint32_t i = threadIdx.x; i < wpf; i += blockDim.x) {
        const uint32_t v = all ? 0xFFFFFFFFu : bits[i];
        if (v != 0u && (out[i] & v) != v) atomicOr(&out[i], v);  // (a stale read only costs the atomic)
    }
}

// The plane pointers of an AOV launch, into the slot's table.
__global__ void prepare_aov_kernel(AovTable tbl, AovDesc* planes) {
    const int i = threadIdx.x;
    if (i < tbl.n) planes[tbl.first + i] = tbl.f[i];
}

// Probe circle overlay, volrend.cu:100-134.  Pixels inside the circle skip the
// ray march (enable_draw=false) and end with alpha 1, so they are independent of
// the main kernel's result and simply overwrite it.  One thread per pixel of the
// (probe_disp_size+5)^2 corner square.
template <int FMA>
__global__ void probe_overlay_kernel(const KParams p) {
    using P = Policy<FMA>;
    const int side = p.probe_disp_size + 5;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= side * side) return;
    const int y = idx / side;
    const int x = p.width - side + (idx - y * side);
    if (x < 0 || x >= p.width || y >= p.height) return;
    // which tile / rank owns this pixel
    const int tx = x / p.tile_w, ty = y / p.tile_h;
    const int tile = ty * p.tiles_x + tx;
    if (tile % p.world != p.rank) return;
    float cen[3], dir[3], out[4] = {0.f, 0.f, 0.f, 0.f};
    const int xx = x - (p.width - p.probe_disp_size) + 5;
    const int yy = y - 5;
    cen[0] = -((float)xx / (0.5f * (float)p.probe_disp_size) - 1.f);
    cen[1] = ((float)yy / (0.5f * (float)p.probe_disp_size) - 1.f);
    const float c = P::madd(cen[0], cen[0], cen[1] * cen[1]);
    if (!(c <= 1.f)) return;
    if (p.basis_dim >= 0) {
        float basis_fn[VR_MAX_BASIS];
#pragma unroll
        for (int i = 0; i < VR_MAX_BASIS; ++i) basis_fn[i] = 0.f;
        cen[2] = -__builtin_sqrtf(1 - c);
        float xf[9];
        for (int i = 0; i < 9; ++i) xf[i] = p.frames[blockIdx.y].xf[i];
        mv3<FMA>(xf, cen, dir);
        precalc_basis<FMA, true>(p, dir, basis_fn);
        // upstream indexes past basis_dim with the default basis_minmax {0,24} (UB);
        // like the oracle, clamp to the coefficients that exist
        int hi = p.basis_max;
        if (hi > p.basis_dim - 1) hi = p.basis_dim - 1;
        const int lo = p.basis_min < 0 ? 0 : p.basis_min;
        for (int tt = 0; tt < 3; ++tt) {
            const int off = tt * p.basis_dim;
            float tmp = 0.f;
            for (int i = lo; i <= hi; ++i) tmp = P::madd(basis_fn[i], p.probe_coeffs[off + i], tmp);
            out[tt] = sigmoid(tmp);
        }
    } else {
        for (int i = 0; i < 3; ++i) out[i] = p.probe_coeffs[i];
    }
    out[3] = 1.f;
    const int64_t pix = (int64_t)y * p.width + x;
    const FrameDesc& fd = p.frames[blockIdx.y];
    if (fd.accum) reinterpret_cast<float4*>(fd.accum)[pix] = make_float4(out[0], out[1], out[2], out[3]);
    // nalpha = 1 - out[3] = 0: the composite adds (+0 * anything) and leaves out[] as is
    uint8_t* const px = pixel_address(p, fd, tile / p.world, x - tx * p.tile_w, y - ty * p.tile_h, x, y);
    *reinterpret_cast<uint32_t*>(px) =
        quant8(out[0]) | (quant8(out[1]) << 8) | (quant8(out[2]) << 16) | 0xFF000000u;
}

// retrieve_cursor_lumisphere_kernel, volrend.cu:175-191
__global__ void probe_kernel(const KParams p, float probe0, float probe1, float probe2,
                             float* out) {
    float cen[3] = {p.offset[0] + p.scale[0] * probe0, p.offset[1] + p.scale[1] * probe1,
                    p.offset[2] + p.scale[2] * probe2};
    float cube_sz;
    int levels;
    uint32_t word;
    const int64_t leaf = query_generic<0>(p, cen, &cube_sz, &levels, &word);
    const uint16_t* v = p.leaves + leaf * p.leaf_stride_h;
    for (int i = threadIdx.x; i < p.data_dim - 1; i += blockDim.x) out[i] = h2f(v[i]);
}

// grid = the persistent waves (persistent_grid, vr_internal.h): as many as the chip holds of this flavour
// (or the tuning override)
// planes: none (colour), or the AovParams of an AOV launch -- the extra kernel argument of its flavours
template <int FMA, int MODE, typename... PLANES>
hipError_t launch_basis(const KParams& p, int64_t total_blocks, int n_cus, int waves_override, hipStream_t s,
                        const PLANES&... planes) {
    const dim3 block(kWave);
    constexpr bool kAov = sizeof...(PLANES) != 0;
#define VR_LAUNCH(B)                                                                         \
    do {                                                                                     \
        const dim3 grid(persistent_grid(total_blocks, n_cus,                                 \
                                        waves_override > 0 ? waves_override : waves_per_cu<B, MODE, kAov>())); \
        constexpr bool kBlk = MODE == MODE_FAST;                                             \
        if (kBlk && p.brick_blocked)                                                         \
            hipLaunchKernelGGL((render_kernel<FMA, B, MODE, kBlk, PLANES...>), grid, block, 0, s, p, planes...); \
        else                                                                                 \
            hipLaunchKernelGGL((render_kernel<FMA, B, MODE, false, PLANES...>), grid, block, 0, s, p, planes...); \
    } while (0)
    switch (basis_flavour(p.format, p.basis_dim)) {
        case BASIS_RGBA: VR_LAUNCH(BASIS_RGBA); break;
        case BASIS_25: VR_LAUNCH(BASIS_25); break;
        case BASIS_16: VR_LAUNCH(BASIS_16); break;
        case BASIS_9: VR_LAUNCH(BASIS_9); break;
        case BASIS_4: VR_LAUNCH(BASIS_4); break;
        default: VR_LAUNCH(BASIS_1); break;
    }
#undef VR_LAUNCH
    return hipGetLastError();
}

template <int FMA, typename... PLANES>
hipError_t launch_fp(const KParams& p, int64_t total_blocks, int n_cus, int waves_override, hipStream_t s,
                     const PLANES&... planes) {
    if (!uses_lookup(p)) return launch_basis<FMA, MODE_GENERIC>(p, total_blocks, n_cus, waves_override, s, planes...);
    if (needs_full(p)) return launch_basis<FMA, MODE_FULL>(p, total_blocks, n_cus, waves_override, s, planes...);
    return launch_basis<FMA, MODE_FAST>(p, total_blocks, n_cus, waves_override, s, planes...);
}

// Ray generation + the persistent march of one launch (the probe overlay is launch_render's own).
// rays: a ray list takes the place of the frames' pixels (never with AOV planes).
template <typename... PLANES>
hipError_t launch_march(const KParams& p, const CullParams& cull, const HeadParams& head, int fp_mode, int n_cus,
                        int waves_override, int gen_waves, hipStream_t stream, const RayList* rays,
                        const PLANES&... planes) {
    const int64_t total_blocks = p.n_wave_blocks * p.n_frames;
    {   // ray generation: gen_waves wave blocks (8x8 pixels each) per workgroup
        const bool full = needs_full(p);
#define VR_GEN(FMA_, FULL_, GW_)                                                                    \
    do {                                                                                            \
        const dim3 grid_((unsigned)((total_blocks + GW_ - 1) / GW_)), block_(kWave * GW_);          \
        if (rays) {                                                                                 \
            if constexpr (sizeof...(PLANES) == 0 && GW_ >= 4)                                       \
                hipLaunchKernelGGL((raygen_rays_kernel<FMA_, FULL_, GW_>), grid_, block_, 0, stream, p, *rays); \
        }                                                                                           \
        else if (!FULL_ && head.max_rounds > 0)                                                     \
            hipLaunchKernelGGL((raygen_kernel<FMA_, FULL_, GW_, !FULL_, PLANES...>), grid_, block_, 0, stream, p, planes..., cull, head); \
        else hipLaunchKernelGGL((raygen_kernel<FMA_, FULL_, GW_, false, PLANES...>), grid_, block_, 0, stream, p, planes..., cull, head); \
    } while (0)
#define VR_GEN_GW(FMA_, FULL_)                                                                      \
    do {                                                                                            \
        if (gen_waves >= 16) VR_GEN(FMA_, FULL_, 16);                                               \
        else if (gen_waves >= 4 || rays) VR_GEN(FMA_, FULL_, 4);  /* (a list: 16 or 4) */           \
        else VR_GEN(FMA_, FULL_, 1);                                                                \
    } while (0)
        if (fp_mode == VR_FP_FMA) {
            if (full) VR_GEN_GW(1, true); else VR_GEN_GW(1, false);
        } else {
            if (full) VR_GEN_GW(0, true); else VR_GEN_GW(0, false);
        }
#undef VR_GEN_GW
#undef VR_GEN
    }
    // the persistent march (its grid: persistent_grid, vr_internal.h)
    return fp_mode == VR_FP_FMA ? launch_fp<1>(p, total_blocks, n_cus, waves_override, stream, planes...)
                                : launch_fp<0>(p, total_blocks, n_cus, waves_override, stream, planes...);
}

}  // namespace

hipError_t launch_prepare(const KParams& p, const FrameTable& tbl, hipStream_t stream, uint32_t* mask,
                          uint32_t words_per_frame) {
    hipLaunchKernelGGL(prepare_launch_kernel, dim3(1), dim3(64), 0, stream, tbl,
                       const_cast<FrameDesc*>(p.frames), p.queue_head, mask, words_per_frame);
    return hipGetLastError();
}

// one workgroup per (part of the list, frame)
hipError_t launch_block_mask(const KParams& p, const MaskParams& m, hipStream_t stream) {
    if (p.n_frames <= 0 || m.groups_per_frame <= 0) return hipSuccess;
    hipLaunchKernelGGL(block_mask_kernel, dim3((unsigned)m.groups_per_frame, (unsigned)p.n_frames), dim3(256), 0, stream,
                       p, m);
    return hipGetLastError();
}

hipError_t launch_render(const KParams& p, const CullParams& cull, const HeadParams& head, int fp_mode, int n_cus,
                         int waves_override, int gen_waves, hipStream_t stream, const RayList* rays) {
    if (p.n_wave_blocks <= 0 || p.n_frames <= 0) return hipSuccess;
    const hipError_t e = launch_march(p, cull, head, fp_mode, n_cus, waves_override, gen_waves, stream, rays);
    if (e != hipSuccess || !p.enable_probe || p.probe_disp_size <= 0) return e;
    const int side = p.probe_disp_size + 5;
    const dim3 pgrid((unsigned)((side * side + 255) / 256), (unsigned)p.n_frames);
    if (fp_mode == VR_FP_FMA)
        hipLaunchKernelGGL(probe_overlay_kernel<1>, pgrid, dim3(256), 0, stream, p);
    else
        hipLaunchKernelGGL(probe_overlay_kernel<0>, pgrid, dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_prepare_aov(const AovParams& a, const AovTable& tbl, hipStream_t stream) {
    hipLaunchKernelGGL(prepare_aov_kernel, dim3(1), dim3(64), 0, stream, tbl, const_cast<AovDesc*>(a.planes));
    return hipGetLastError();
}

// (no probe overlay: vr_render_aov refuses enable_probe)
hipError_t launch_render_aov(const KParams& p, const AovParams& a, const CullParams& cull, const HeadParams& head,
                             int fp_mode, int n_cus, int waves_override, int gen_waves, hipStream_t stream) {
    if (p.n_wave_blocks <= 0 || p.n_frames <= 0) return hipSuccess;
    return launch_march(p, cull, head, fp_mode, n_cus, waves_override, gen_waves, stream, /* rays */ nullptr, a);
}

hipError_t launch_probe(const KParams& p, const float probe[3], float* out_dev,
                        hipStream_t stream) {
    hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(64), 0, stream, p, probe[0], probe[1],
                       probe[2], out_dev);
    return hipGetLastError();
}

}  // namespace vr
