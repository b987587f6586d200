// vr_query.h -- shared between the host side of vr_query_points / vr_query_grid (vr_query.cpp) and
// their kernels (vr_query.hip).  Not part of the public ABI.
#pragma once
#include "vr_internal.h"

namespace vr {

constexpr int64_t kMaxGridCells = 1ll << 40;  // vr_query_grid: res[0] * res[1] * res[2]

// Where the points of a query come from.
enum { kPointsArray = 0, kPointsGrid = 1 };

// One bulk query, passed BY VALUE next to KParams (of which only the tree part is filled in).
// The points are handed out in CHUNKS of up to 64 consecutive output indices, one per wave:
//   array: chunk c = points [64 c, 64 c + 64)
//   grid : chunk c = 64 consecutive k of one (i, j) row; c = (i * k_blocks + kb) * res[1] + j, so
//          that the chunks a wave takes one after the other are neighbours in j and a lane's
//          consecutive points mostly share their top cell (query_n2's Cursor).
struct QueryArgs {
    const float* xyz;    // array: [n][3]
    const float* dirs;   // array: [n][3] or NULL
    float lo[3];         // grid: coordinate of cell i = lo + ((float)i + 0.5f) * cell
    float cell[3];       // grid: (hi - lo) / (float)res, rounded once per operator on the host
    float dir[3];        // grid: the one direction (zeros when none is given: rgb is refused then)
    int32_t res[3];
    int32_t k_blocks;    // grid: (res[2] + 63) / 64
    int32_t space;       // VR_SPACE_*
    int32_t coeffs_vec4; // the records leave as float4: data_dim - 1 is a multiple of 4 and coeffs is 16-byte aligned
    int64_t n;           // points
    int64_t n_chunks;
    float* sigma;        // VrQueryOut
    int32_t* depth;
    float* local;
    float* coeffs;
    float* rgb;
};

// vr_query.hip
hipError_t launch_query(const KParams& p, const QueryArgs& q, int source, int n_cus, hipStream_t stream);

}  // namespace vr
