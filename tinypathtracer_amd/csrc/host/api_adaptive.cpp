// api_adaptive.cpp -- tpt_render_adaptive of the C-ABI: passes of k_trace over the list of
// tiles still above the target (listed launches, trace.hip), the error estimate and the
// per-tile resolve (adaptive.hip).  DESIGN.md section 5 "Adaptive sampling".
#include <chrono>
#include <cmath>

#include "api_internal.hpp"

extern "C" {

tpt_status tpt_render_adaptive(tpt_scene* s, const tpt_env* env, const tpt_camera* cam, const tpt_params* p,
                               const tpt_adaptive_params* ap, float* radiance_out, uint8_t* bgra_out,
                               int32_t* tile_spp_out, float* tile_error_out, tpt_adaptive_stats* stats) {
    auto t_start = std::chrono::steady_clock::now();
    if (!s || !cam || !p || !ap) return fail(TPT_ERR_INVALID_ARG, "null argument");
    if (!s->built) return fail(TPT_ERR_INVALID_ARG, "scene not built (call tpt_scene_build)");
    if (p->width <= 0 || p->height <= 0 || p->max_depth < 1 || p->max_depth > 64)
        return fail(TPT_ERR_INVALID_ARG, "bad frame parameters");
    if ((int64_t)p->width * p->height > (int64_t)1 << 30) return fail(TPT_ERR_INVALID_ARG, "frame too large");
    if (p->width > 16 * 65536 || p->height > 16 * 65536)
        return fail(TPT_ERR_INVALID_ARG, "adaptive: at most 65,536 tiles each way");
    if (env && env->device != s->device) return fail(TPT_ERR_INVALID_ARG, "env lives on another device");
    if (ap->min_spp < 2 || ap->min_spp % 2 != 0) return fail(TPT_ERR_INVALID_ARG, "adaptive: min_spp even and >= 2");
    {
        int64_t n = ap->min_spp;
        while (n < (int64_t)ap->max_spp) n *= 2;
        if (n != (int64_t)ap->max_spp) return fail(TPT_ERR_INVALID_ARG, "adaptive: max_spp = min_spp * 2^j");
    }
    if (!(ap->target >= 0.0f)) return fail(TPT_ERR_INVALID_ARG, "adaptive: target >= 0 (+inf allowed)");
    if (ap->flags != 0) return fail(TPT_ERR_INVALID_ARG, "adaptive: unknown flags");
    if (p->flags & (TPT_FLAG_WAVEFRONT | TPT_FLAG_ACCUMULATE))
        return fail(TPT_ERR_INVALID_ARG, "adaptive: not with TPT_FLAG_WAVEFRONT or TPT_FLAG_ACCUMULATE");
    if (p->band_count > 1 || p->band_index != 0 || p->band_list || p->band_list_len != 0 || p->band_cost)
        return fail(TPT_ERR_INVALID_ARG, "adaptive: the whole frame only (no bands, band list or band_cost)");
    if (!radiance_out && !bgra_out) return fail(TPT_ERR_INVALID_ARG, "adaptive: no image output");

    const int W = p->width, H = p->height;
    const int tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16;
    const size_t n_tiles = (size_t)tiles_x * (size_t)tiles_y, npix = (size_t)W * (size_t)H;
    DeviceGuard g(s->device);
    hipStream_t st = s->stream;

    s->acc_valid = false;   // the streams and sums are this call's: tiles end at different counts
    HIP_OR_FAIL(s->rng.alloc(6 * npix));
    HIP_OR_FAIL(s->accum.alloc(3 * npix));
    HIP_OR_FAIL(s->counters.alloc(32));
    HIP_OR_FAIL(s->ad_snap.alloc(3 * npix));
    HIP_OR_FAIL(s->ad_err.alloc(n_tiles));
    HIP_OR_FAIL(s->ad_tiles.alloc(n_tiles));
    HIP_OR_FAIL(s->ad_spp.alloc(n_tiles));
    HIP_OR_FAIL(s->ad_err_h.alloc(n_tiles));
    HIP_OR_FAIL(s->ad_tiles_h.alloc(n_tiles));
    HIP_OR_FAIL(s->ad_spp_h.alloc(n_tiles));
    HIP_OR_FAIL(hipMemsetAsync(s->accum.p, 0, 3 * npix * sizeof(float), st));
    HIP_OR_FAIL(hipMemsetAsync(s->counters.p, 0, 32 * sizeof(unsigned long long), st));
    HIP_OR_FAIL(hipMemsetAsync(s->ad_err.p, 0, n_tiles * sizeof(float), st));
    HIP_OR_FAIL(tpt::launch_rng_init(s->jumps.p, p->seed, W, 16, 1, 0, nullptr, H, H, s->rng.p, st));
    {
        const tpt_status bs = finish_pending(s, nullptr);
        if (bs != TPT_OK) return bs;
    }

    tpt::TraceArgs a{};
    fill_trace_args(s, env, cam, a);
    a.inv_w = 1.0f / (float)W;
    a.inv_h = 1.0f / (float)H;
    a.width = W;
    a.height = H;
    a.band_rows = 16;
    a.band_count = 1;
    a.band_index = 0;
    a.band_height = H;
    a.n_frames = 1;
    a.max_depth = p->max_depth;
    a.flags = p->flags;
    if (p->flags & (TPT_FLAG_APPROX_CULL | TPT_FLAG_FAST)) {   // as tpt_render
        a.cull_eps = 0.0f;
        a.n_sliver_groups = 0;
        a.graze = 0;
    }
    a.env_is = ((p->flags & TPT_FLAG_ENV_IS) && env && env->is_total > 0.0f) ? 1 : 0;
    a.rng = s->rng.p;
    a.accum = s->accum.p;
    a.counters = s->counters.p;
    a.tile_list = s->ad_tiles.p;

    tpt::PlanInput pin;
    pin.width = W;
    pin.bh = H;
    pin.height = H;
    pin.flags = p->flags;
    pin.lanes_per_pixel = p->lanes_per_pixel;
    pin.refill = p->refill;
    pin.leaf_batch = p->leaf_batch;
    pin.n_faces = s->n_faces;
    pin.n_lights = s->n_lights;
    pin.n_materials = s->n_materials;
    pin.resident_lanes = s->resident_lanes;
    pin.env_is = a.env_is != 0;
    pin.quad_fits = tpt::trace_quad_fits(a);
    pin.max_depth = p->max_depth;
    pin.any_emitter = s->any_emitter != 0;

    // the active tiles, in the dispatch order of an unlisted launch (row by row from the bottom)
    uint32_t* const list = s->ad_tiles_h.p;
    int32_t* const spp = s->ad_spp_h.p;
    size_t n_active = n_tiles;
    for (int ty = 0; ty < tiles_y; ++ty)
        for (int tx = 0; tx < tiles_x; ++tx) list[(size_t)ty * tiles_x + tx] = (uint32_t)tx | (uint32_t)ty << 16;
    auto tile_of = [&](uint32_t t) { return (size_t)(t >> 16) * (size_t)tiles_x + (size_t)(t & 0xffffu); };

    double trace_ms = 0.0, error_ms = 0.0;
    int passes = 0;
    // one pass: `samples` more for every active tile (the list is on the device), then the snapshot
    // (estimate_n 0) or the estimate at estimate_n samples; returns with the stream drained
    auto pass = [&](int samples, int estimate_n) -> tpt_status {
        pin.n_tiles = (int32_t)n_active;
        pin.spp = samples;
        const tpt::LaunchPlan plan = tpt::plan_launches(pin);
        if (plan.status != TPT_OK) return fail(plan.status, plan.message);
        a.pair = plan.pair ? 1 : 0;
        a.quad = plan.quad ? 1 : 0;
        a.refill = plan.refill;
        a.drained = plan.drained ? 1 : 0;
        a.leaf_kb = plan.leaf_kb;
        a.xcd_run = 0;
        a.n_tiles = (int32_t)n_active;
        HIP_OR_FAIL(hipMemcpyAsync(s->ad_tiles.p, list, n_active * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_OR_FAIL(hipEventRecord(s->ev[0], st));
        for (size_t oi = 0; oi < plan.order.size(); ++oi) {
            a.samples = plan.launches[plan.order[oi]].samples;
            HIP_OR_FAIL((p->flags & TPT_FLAG_FAST) ? tpt_fast::launch_trace_ptr(&a, st, nullptr)
                                                   : tpt::launch_trace(a, st, nullptr));
        }
        HIP_OR_FAIL(hipEventRecord(s->ev[1], st));
        tpt::TileErrorArgs e{};
        e.accum = s->accum.p;
        e.snapshot = s->ad_snap.p;
        e.tile_list = s->ad_tiles.p;
        e.tile_error = s->ad_err.p;
        e.n_tiles = (int32_t)n_active;
        e.width = W;
        e.height = H;
        e.tiles_x = tiles_x;
        e.n = estimate_n;
        e.snapshot_only = estimate_n == 0 ? 1 : 0;
        HIP_OR_FAIL(tpt::launch_tile_error(e, st));
        HIP_OR_FAIL(hipEventRecord(s->ev[2], st));
        if (estimate_n)
            HIP_OR_FAIL(hipMemcpyAsync(s->ad_err_h.p, s->ad_err.p, n_tiles * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_OR_FAIL(hipStreamSynchronize(st));
        float ms = 0.0f;
        HIP_OR_FAIL(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
        trace_ms += ms;
        HIP_OR_FAIL(hipEventElapsedTime(&ms, s->ev[1], s->ev[2]));
        error_ms += ms;
        ++passes;
        return TPT_OK;
    };

    int n = ap->min_spp, unconverged = 0;
    tpt_status ts = pass(n / 2, 0);
    if (ts == TPT_OK) ts = pass(n / 2, n);
    while (ts == TPT_OK) {
        // the stop rule: E < target stops the tile (NaN never does); at max_spp the rest stop unconverged
        size_t kept = 0;
        for (size_t i = 0; i < n_active; ++i) {
            const uint32_t t = list[i];
            if (s->ad_err_h.p[tile_of(t)] < ap->target) {
                spp[tile_of(t)] = n;
            } else if (n == ap->max_spp) {
                spp[tile_of(t)] = n;
                ++unconverged;
            } else {
                list[kept++] = t;
            }
        }
        n_active = kept;
        if (n_active == 0) break;
        ts = pass(n, 2 * n);   // the snapshot is at n: n more samples, the estimate at 2n
        n *= 2;
    }
    if (ts != TPT_OK) {
        // An error in the middle of a pass must not leave its earlier launches writing the rng, sum and
        // snapshot planes, or the upload still reading the pinned list, behind the caller's back: drain
        // the stream before failing (as render_planned joins its sets).
        (void)hipStreamSynchronize(st);
        return ts;
    }

    unsigned long long cnt[32] = {0};
    HIP_OR_FAIL(hipMemcpyAsync(cnt, s->counters.p, sizeof cnt, hipMemcpyDeviceToHost, st));
    HIP_OR_FAIL(hipStreamSynchronize(st));
    if (cnt[4] != 0) return fail(TPT_ERR_HIP, "traversal stack overflow (BVH deeper than sized)");

    // the resolve at each tile's own count, then the outputs
    HIP_OR_FAIL(hipMemcpyAsync(s->ad_spp.p, spp, n_tiles * sizeof(int32_t), hipMemcpyHostToDevice, st));
    Staging sg(st);
    tpt::ResolveTilesArgs r{};
    r.accum = s->accum.p;
    r.tile_spp = s->ad_spp.p;
    r.width = W;
    r.height = H;
    r.tiles_x = tiles_x;
    // (the caller's bytes go up first: the resolve writes no alpha)
    HIP_OR_FAIL(sg.out(s->radiance_tmp, radiance_out, 3 * npix, &r.radiance));
    HIP_OR_FAIL(sg.inout(s->bgra_tmp, bgra_out, 4 * npix, &r.bgra));
    HIP_OR_FAIL(tpt::launch_resolve_tiles(r, st));
    HIP_OR_FAIL(sg.finish());
    if (tile_spp_out)
        HIP_OR_FAIL(hipMemcpyAsync(tile_spp_out, s->ad_spp.p, n_tiles * sizeof(int32_t), hipMemcpyDefault, st));
    if (tile_error_out)
        HIP_OR_FAIL(hipMemcpyAsync(tile_error_out, s->ad_err.p, n_tiles * sizeof(float), hipMemcpyDefault, st));
    HIP_OR_FAIL(hipStreamSynchronize(st));

    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx)
                stats->samples += (uint64_t)std::min(16, W - 16 * tx) * (uint64_t)std::min(16, H - 16 * ty) *
                                  (uint64_t)spp[(size_t)ty * tiles_x + tx];
        stats->pixels = (uint64_t)npix;
        stats->traversals = cnt[0];
        stats->passes = passes;
        stats->unconverged_tiles = unconverged;
        stats->trace_ms = trace_ms;
        stats->error_ms = error_ms;
        stats->total_ms =
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return TPT_OK;
}

}  // extern "C"
