// launch_plan.hpp -- how tpt_render_frames launches k_trace: the lane mode, the
// kernel's batching knobs, the XCD run length and the schedule of launches over
// band sets and sample chunks.  Pure integer arithmetic on the call's
// parameters (no HIP, no scene access), so the host compiler builds it alone
// and the rules are testable without a GPU (tests/sanitize/host_check.cpp
// "plan").  launch_plan.cpp holds the rules and their measurements.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../common/trace_variant.hpp"
#include "tpt.h"

namespace tpt {

constexpr int kMaxPipe = 4;         // overlapped launch sets per frame (GPU_MAX_HW_QUEUES is 4)
constexpr int kPipeMinChunk = 128;  // spp per pipelined launch, at least

// rows of the interleaved deal's band `band_index` of `band_count`
int band_height_of(int height, int band_rows, int band_count, int band_index);
// rows of an explicit deal: the bands `list[0, n)` (only the frame's last band can be short)
int band_list_rows(const int32_t* list, size_t n, int band_rows, int height);

struct PlanInput {
    int32_t width = 0, band_rows = 16;
    int32_t bh = 0;                     // rows this call renders (band_height_of / band_list_rows)
    int32_t height = 0, n_frames = 1;
    int32_t band_count = 1, band_index = 0;
    bool listed = false;                // an explicit deal: band_count 1, band_index 0
    const int32_t* list = nullptr;      // its validated band ids
    size_t list_len = 0;
    // tpt_params
    int32_t spp = 0, flags = 0, lanes_per_pixel = 0, refill = 0, leaf_batch = 0, spp_per_launch = 0, pipe_sets = 0,
            pipe_chunks = 0;
    // the scene
    int32_t n_faces = 0, n_lights = 0, n_materials = 0;
    uint64_t resident_lanes = 0;
    bool env_is = false;                // TPT_FLAG_ENV_IS and an env with a non-empty distribution
    bool quad_fits = false;             // tpt::trace_quad_fits of the call's TraceArgs
    int32_t max_depth = 8;              // tpt_params
    bool any_emitter = true;            // some triangle of the scene emits
    // >= 0: a listed launch over this many 16x16-pixel tiles of the whole frame (TraceArgs tile_list;
    // tpt_render_adaptive): the lane-mode and drained-launch rules key on 256 * n_tiles pixels, no XCD
    // runs, one band set on one stream, its spp chunked as for one set
    int32_t n_tiles = -1;
};

struct PlanLaunch {
    int32_t set, samples;
    int32_t ahead_max = 0;              // the samples of the same set's later launches (TraceArgs::ahead_max)
};

struct LaunchPlan {
    tpt_status status = TPT_OK;         // TPT_ERR_INVALID_ARG: message says why, nothing else is set
    const char* message = "";
    bool pair = false;                  // TraceArgs::pair
    bool pair_kernel = false;           // a two-lane variant really runs (else the kernel falls back to one lane)
    bool quad = false, drained = false;
    int32_t refill = 0, leaf_kb = 0, xcd_run = 0;
    int32_t wg_rows = 16;               // rows of a trace workgroup (the grid's y extent)
    // the schedule (empty for TPT_FLAG_WAVEFRONT, which has none)
    int32_t nset = 1, chunk = 0;
    std::vector<PlanLaunch> launches;   // set by set, each set's chunks in order
    std::vector<size_t> order;          // indices into launches, in issue order
    int32_t set_rows[kMaxPipe] = {};    // rows of set k
    // an explicit deal over nset > 1 sets: set k's share of the list, and where it
    // lies in the device copy (the whole list first, then the shares of sets 0, 1, ...)
    std::vector<int32_t> set_list[kMaxPipe];
    size_t set_off[kMaxPipe] = {};
};

LaunchPlan plan_launches(const PlanInput& in);

}  // namespace tpt
