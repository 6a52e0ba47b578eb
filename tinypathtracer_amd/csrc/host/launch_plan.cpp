// launch_plan.cpp -- the launch rules of tpt_render_frames (launch_plan.hpp), with
// the measurements each default rests on.
#include "launch_plan.hpp"

#include <algorithm>
#include <cmath>

namespace tpt {

int band_height_of(int height, int band_rows, int band_count, int band_index) {
    int n = 0;
    for (int y = 0; y < height; ++y)
        if ((y / band_rows) % band_count == band_index) ++n;
    return n;
}

int band_list_rows(const int32_t* list, size_t n, int band_rows, int height) {
    int rows = 0;
    for (size_t i = 0; i < n; ++i) rows += std::min(band_rows, height - list[i] * band_rows);
    return rows;
}

static LaunchPlan plan_error(const char* message) {
    LaunchPlan pl;
    pl.status = TPT_ERR_INVALID_ARG;
    pl.message = message;
    return pl;
}

LaunchPlan plan_launches(const PlanInput& in) {
    LaunchPlan pl;
    const int W = in.width, H = in.height, bh = in.bh, band_rows = in.band_rows;
    const size_t nf = (size_t)in.n_frames;
    const bool lit = in.n_lights > 0 || in.env_is;
    const bool ref_order = (in.flags & TPT_FLAG_REF_ORDER) != 0;

    if (in.lanes_per_pixel < 0 || in.lanes_per_pixel > 4 || in.lanes_per_pixel == 3)
        return plan_error("lanes_per_pixel: 0, 1, 2 or 4");
    // auto: pair mode wherever there are shadow rays to hand off (C3 1080p 4096 spp:
    // 4.91 -> 6.65 Grays/s); the kernel falls back to one lane per pixel otherwise
    // (A15 env IS: the env shadow ray of every diffuse bounce is the side lane's job too)
    pl.pair = in.lanes_per_pixel == 2 || (in.lanes_per_pixel == 0 && lit);
    // Four lanes per pixel ("Four lanes per ray"): every lane
    // of a quad runs the pixel's path, each 4-wide visit split over them -- the
    // one-lane kernel logic, so no delta lights, env IS or reference order, and the
    // quads' stacks in LDS.  Auto on launches with no more pixels than the chip's
    // resident lanes (resident_lanes, from the device: MI355X 256 CUs x 4 SIMDs x
    // 5 waves x 64 = 327,680), which are their heaviest tiles' serial chains:
    // strong-scaled C2 at N = 8 (259 K pixels per GPU, slowest rank) 314 -> 250 ms;
    // at N = 4 (518 K) four lanes lose (463 vs 328 ms: four times the waves), so
    // the chip is the bound.
    const bool tiles = in.n_tiles >= 0;   // a listed launch
    if (tiles && ((in.flags & TPT_FLAG_WAVEFRONT) || in.listed || in.band_count != 1 || in.band_index != 0 || nf != 1 || bh != H))
        return plan_error("a tile list takes the whole frame: one frame, no bands, not the wavefront variant");
    const double launch_pix =
        tiles ? 256.0 * (double)std::max(in.n_tiles, 1) : (double)W * (double)std::max(bh, 1) * (double)nf;
    const double resident = (double)in.resident_lanes;
    // (the wavefront variant has no lane modes: tpt.h, lanes_per_pixel is not used there)
    const bool wavefront = (in.flags & TPT_FLAG_WAVEFRONT) != 0;
    const bool quad_ok = !wavefront && in.lanes_per_pixel != 2 && !lit && !ref_order && in.quad_fits;
    if (in.lanes_per_pixel == 4 && !quad_ok && !wavefront)
        return plan_error("lanes_per_pixel 4: scenes without delta lights, no env IS, ordered traversal, stacks in LDS");
    pl.quad = in.lanes_per_pixel == 4 || (in.lanes_per_pixel == 0 && launch_pix <= resident && quad_ok);
    // A launch with fewer pixels than about twice the chip's resident lanes
    // (resident_lanes; strong-scaled frames, small images) is bound by its
    // heaviest waves' chains, not by throughput: batch the shading passes harder
    // (C2 rank 0 of 8: refill 24 318 ms, 4: 276 ms; rank 0 of 4: flat).
    pl.drained = launch_pix < 2.0 * resident;   // latency-oriented kernel variants (trace.hip DRAIN)
    // what launch_trace will pick, by its own rule (a request it refuses was reported above)
    const TraceKey variant = select_trace_variant({ref_order, in.env_is, pl.pair, pl.quad, pl.drained, in.n_lights,
                                                   in.n_materials, in.n_faces, in.max_depth, in.any_emitter}).key;
    pl.pair_kernel = kTraceFamily[variant.family].lanes == 2;
    pl.wg_rows = kTraceFamily[variant.family].tile_rows;   // the trace grid's y extent is (band row blocks) x frames
    if (!wavefront && !tiles && (size_t)((bh + pl.wg_rows - 1) / pl.wg_rows) * nf > 65535)
        return plan_error("frame batch too large for one launch");
    // Shallow trees (few triangles) make a traversal short against a shading
    // pass, so passes are batched harder there: tir (6 triangles) refill 16
    // 84.6 Grays/s vs 24 72.6-78.9; box (1,932) 16 = 24; C5 (131 K) 16 -3 %.
    const int full = in.n_faces <= 4096 ? 16 : 24;
    // Refill: a wave leaves its traversal loop to shade once fewer than this many
    // lanes still traverse.  A shading pass costs ~5 node steps, so passes are
    // batched; in pair mode half the lanes (the side lanes) are mostly idle and
    // the threshold scales down with them (C3 1080p 4096 spp: 24 -> 5.88,
    // 8 -> 6.44, 2..12 within 6.2-6.6 Grays/s; C2 single-lane: 16-24 best).
    // Pair mode (round 3, after the 4-wave pair variants and the fp32-bounded env
    // lookup; C3 1080p 4096 spp, Mrays/s): refill 8 7,711, 6 7,720, 4 7,790-7,942,
    // 3 7,911-7,934, 2 7,860-7,983 -> 3; with env IS (the side lane's env sample
    // and shadow ray per diffuse bounce): 8 5,562-5,630, 4 5,745-5,803, 2
    // 5,934-5,970, 1 6,070-6,153 -> 1 (the wave shades only once no lane traverses).
    // Round 5, after the emitter-free pair variants (C3, 2 reps): 4 8,071 / 8,129,
    // 3 8,185 / 8,156, 2 8,223 / 8,260, 1 8,676 / 8,710 -> 1 without env IS too.
    pl.refill = in.refill > 0 ? std::min(in.refill, 64) : (pl.pair_kernel ? 1 : (pl.drained ? 4 : full));
    // Parked-leaf batch (speculative leaf postponement): a wave runs its triangle
    // tests once this many lanes are blocked on a parked leaf.  Pair mode has
    // half the path lanes and its heavy waves few traversing lanes, so it
    // batches less (C3 4096 spp: 4 -> 6.84, 2 -> 7.45, 8 -> 5.86 Grays/s;
    // C2, C4 and C5 within 2 % either way).
    // Drained launches likewise (strong-scaled C2, rank 0 of 8: 4 -> 259 ms, 2 -> 252 ms, 8 -> 277 ms).
    // Re-swept at the end of round 3 with the new pair refill (C3: 1 -> 7,988-8,092,
    // 2 -> 7,826-7,886, 3 -> 7,414-7,457 Mrays/s; C3 + IS: 1 -> 6,191-6,212,
    // 2 -> 6,111-6,133): 1 in pair mode.
    pl.leaf_kb = in.leaf_batch > 0 ? std::min(in.leaf_batch, 64) : (pl.pair_kernel ? 1 : (pl.drained ? 2 : 4));
    // XCD runs (trace.hip k_trace prologue) for scenes that do not fit one XCD's
    // 4 MiB L2 (≈ 200 B of nodes, triangles and shading data per face): the
    // largest run length <= 10 that divides a row's tiles per XCD (C5 3840 px:
    // 10 +4.1 %, 30 +3.7 %, 5 +2.1 %, 3 +1.9 %).
    pl.xcd_run = 0;
#ifndef TPT_XCD_RUNS_OFF   // (A/B builds: round-robin workgroups on every scene)
    if (in.n_faces > 16384 && !tiles) {
        const int gx = (W + 15) / 16, per = gx / 8;
        if (gx % 8 == 0)
            for (int g = std::min(per, 10); g >= 2 && pl.xcd_run == 0; --g)
                if (per % g == 0) pl.xcd_run = g;
    }
#endif
    for (int k = 0; k < kMaxPipe; ++k) pl.set_rows[k] = k == 0 ? bh : 0;
    if (wavefront) return pl;

    // Launch schedule.  A launch ends in a tail where CUs drain: a wave's life
    // is its heaviest pixel's serial chain (samples run in order on one lane),
    // and the waves dispatched last (the top rows of the box) live ~40x longer
    // than the miss tiles -- measured on box at 256 spp, 25 % of the launch's
    // wave slots idle.  Default (spp >= 1024): the rows split into P = 3 interleaved band sets,
    // each on its own stream, and the spp into chunks, set k's chunk boundaries
    // offset by k/P of a chunk: while one set's launch drains, another set's
    // launch is mid-flight and takes the freed slots.  A pixel's samples still
    // run in order (its set's launches are stream-ordered, RNG and sums persist
    // between chunks), so the result is bit-identical to one launch.
    // params pipe_sets (1: one stream) and pipe_chunks (chunks per set) override;
    // an explicit spp_per_launch keeps the single-stream chunked loop.
    int chunk = in.spp_per_launch;
    int nset = 1;
    if (chunk <= 0) {
        // one stream: chunk only past ~4096 spp of 1080p pixels so one launch stays below ~5 s
        // (clamped: below 4 pixels the quotient is past an int)
        chunk = (int)std::min(2147483647.0, std::max(1.0, std::floor(4096.0 * 2073600.0 / launch_pix)));
        const bool forced = in.pipe_sets > 0;
        nset = tiles ? 1 : (forced ? in.pipe_sets : 3);
        // (pair mode: 16 -- C3 4096 spp, 256-spp chunks: 8,180 vs 8,016-8,032 Mrays/s with 8,
        // 7,743 with 4; C3 + IS 6,322 vs 6,206-6,267)
        const int per_set = in.pipe_chunks > 0 ? in.pipe_chunks : (pl.pair_kernel ? 16 : 8);
        nset = std::max(1, std::min(nset, kMaxPipe));
        // worth it only with several chunks of real work and rows for every set
        if (bh < nset * band_rows) nset = 1;
        // chunks of at least 128 spp, and by default only from 1024 spp on
        // (measured on box 1080p, 3 sets: 1024 spp +6.7 %; 256 spp -2 %, 32-spp
        // chunks -4 %: concurrently running launches at different rows cost
        // locality, and every launch its prologue)
        // (both pipe_sets and pipe_chunks given: exactly that schedule, any chunk
        // size -- tests run the pipeline at full resolution and a few spp)
        const bool exact = forced && in.pipe_chunks > 0;
        const int min_chunk = exact ? 1 : kPipeMinChunk;
        if (nset > 1) chunk = std::min(chunk, std::max(min_chunk, (in.spp + per_set - 1) / per_set));
        if (!exact && in.spp < (forced ? 2 : 8) * kPipeMinChunk) nset = 1;
    }
    chunk = std::min(chunk, in.spp);
    pl.nset = nset;
    pl.chunk = chunk;
    for (int k = 0; k < nset; ++k) {
        int done = 0;
        const int first = chunk - (k * chunk) / nset;   // set k starts k/nset of a chunk early
        for (int c = first; done < in.spp && bh > 0; c = chunk) {
            const int n = std::min(c, in.spp - done);
            pl.launches.push_back({k, n});
            done += n;
        }
    }
    // what each launch's set still has to give after it (launches lie set by set, in order)
    for (size_t j = pl.launches.size(); j-- > 1;)
        if (pl.launches[j - 1].set == pl.launches[j].set)
            pl.launches[j - 1].ahead_max = pl.launches[j].samples + pl.launches[j].ahead_max;
    // set k renders bands band_index + k * band_count of the band_count * nset
    // interleave; of an explicit deal, list entries k, k + nset, ... (a short last
    // band, last in the list, stays last in its set)
    for (int k = 0; k < nset && nset > 1; ++k) {
        if (in.listed) {
            std::vector<int32_t>& sub = pl.set_list[k];
            for (size_t i = (size_t)k; i < in.list_len; i += (size_t)nset) sub.push_back(in.list[i]);
            pl.set_rows[k] = band_list_rows(sub.data(), sub.size(), band_rows, H);
            pl.set_off[k] = in.list_len;   // after the whole list, then the shares of sets 0 .. k-1
            for (int j = 0; j < k; ++j) pl.set_off[k] += (in.list_len + nset - 1 - j) / nset;
        } else {
            pl.set_rows[k] = band_height_of(H, band_rows, in.band_count * nset, in.band_index + k * in.band_count);
        }
    }
    // issue the sets' launches interleaved in time order (chunk starts), so no
    // stream's queue runs ahead of the others on the host side
    pl.order.resize(pl.launches.size());
    std::vector<double> t0(pl.launches.size());
    double at[kMaxPipe] = {};
    for (size_t j = 0; j < pl.launches.size(); ++j) {
        t0[j] = at[pl.launches[j].set];
        at[pl.launches[j].set] += pl.launches[j].samples;
        pl.order[j] = j;
    }
    std::stable_sort(pl.order.begin(), pl.order.end(), [&](size_t x, size_t y) { return t0[x] < t0[y]; });
    return pl;
}

}  // namespace tpt
