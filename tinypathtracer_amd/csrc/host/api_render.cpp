// api_render.cpp -- tpt_render / tpt_render_frames of the C-ABI: the frame's state,
// the trace launches (k_trace over the launch plan of launch_plan.cpp, or the
// wavefront variant), the resolve and the read-back.
//
// Replaces the reference's per-frame orchestration PathTracer::doTrace
// (src/path_tracer.cu:491-554).
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "api_internal.hpp"

#ifndef TPT_XCD_ROT
#define TPT_XCD_ROT 1   // XCD runs rotate by one per chunk of a set (0: every chunk alike; A/B builds)
#endif

void tpt::host::fill_env_args(const tpt_env* env, tpt::TraceArgs& a) {
    a.env = env ? env->texels.p : nullptr;
    a.env_w = env ? env->w : 0;
    a.env_h = env ? env->h : 0;
    a.is_b = env ? env->is_b : 1;
    a.is_bw = env ? env->is_bw : 0;
    a.is_bh = env ? env->is_bh : 0;
    a.is_cond = env ? env->is_cond.p : nullptr;
    a.is_row = env ? env->is_row.p : nullptr;
    a.is_marg = env ? env->is_marg.p : nullptr;
    a.is_total = env ? env->is_total : 0.0f;
    a.is_guide_r = env ? env->is_guide_r.p : nullptr;
    a.is_guide_c = env ? env->is_guide_c.p : nullptr;
    a.is_kr = env ? env->is_kr : 1;
    a.is_kc = env ? env->is_kc : 1;
}

void tpt::host::fill_trace_args(tpt_scene* s, const tpt_env* env, const tpt_camera* cam, tpt::TraceArgs& a) {
    a.inner = s->inner.p;
    a.inner4 = s->inner4.p;
    a.n4 = s->n4;
    a.tri = s->tri.p;
    a.shade = s->shade.p;
    a.mtl = s->mtl.p;
    a.n_faces = s->n_faces;
    a.n_materials = s->n_materials;
    a.n_lights = s->n_lights;
    a.lights = s->lights.p;
    a.stack_depth = s->stack_depth;
    a.boxes_finite = s->boxes_finite;
    a.any_emitter = s->any_emitter;
    a.emit_root = s->emit_root;
    a.unwind_prune = s->unwind_prune;
#ifdef TPT_PROFILE_PHASES
    if (std::getenv("TPT_DEBUG_NO_PRUNE")) a.unwind_prune = 0;   // the unpruned unwind's counts from the same build
#endif
    a.n_emit_box = s->any_emitter ? s->n_emit_box : 0;
    for (int k = 0; k < a.n_emit_box; ++k) {
        const float* b = s->emit_box + 6 * k;
        a.emit_box[2 * k] = make_float4(b[0], b[1], b[2], 0.0f);
        a.emit_box[2 * k + 1] = make_float4(b[3], b[4], b[5], 0.0f);
    }
    a.sliver_groups = s->sliver_groups.p;
    a.sliver_list = s->sliver_list.p;
    a.n_sliver_groups = s->n_sliver_groups;
    a.cull_eps = s->cull_eps;
    a.graze = 1;
    fill_env_args(env, a);
    if (cam) set_camera(a, camera_consts(cam));
}

namespace {

// The wavefront / ray-queue variant (TPT_FLAG_WAVEFRONT; wavefront.hip, DESIGN.md
// section 5 "N1"): every pixel's samples on one slot, in order, so the frame is
// bit-identical to k_trace's.  Slots default to every pixel of the call (the
// whole frame in flight: the fewest iterations); the buffers stay with the
// scene between calls.  The trace phase runs on the scene's stream after the
// RNG initialisation (event ev[1]).
tpt_status render_wavefront(tpt_scene* s, const tpt::TraceArgs& a, const tpt_params* p, int n_frames, int bh,
                            double& trace_ms, double& kernel_ms, int& launches) {
    hipStream_t st = s->stream;
    const bool ordered = !(p->flags & TPT_FLAG_REF_ORDER);
    // the megakernel's record layout: 5 words with delta lights, env IS or the reference order
    const bool lights = tpt::trace_five_words(!ordered, a.env_is != 0, s->n_lights, s->n_materials);
    tpt::WfArgs w{};
    w.t = a;
    w.t.samples = p->spp;
    w.ordered = ordered ? 1 : 0;
    w.state_words = lights ? 32 : 16;
    w.rec_words = lights ? 5 : 2;
    const size_t gx = (size_t)(p->width + 15) / 16, gy = (size_t)((bh + 15) / 16) * (size_t)n_frames;
    const size_t claims = gx * gy * 256;
    if (bh <= 0) return TPT_OK;
    if (claims > (size_t)INT32_MAX / 2) return fail(TPT_ERR_INVALID_ARG, "wavefront: frame batch too large");
    if (p->wf_slots < 0 || p->wf_refill < 0 || p->wf_refill > 64)
        return fail(TPT_ERR_INVALID_ARG, "wavefront: wf_slots >= 0, wf_refill 0..64");
    size_t slots = p->wf_slots > 0 ? (size_t)p->wf_slots : claims;
    slots = std::min(slots, claims);
    slots = (slots + 255) / 256 * 256;
    w.n_claims = (int32_t)claims;
    w.n_slots = (int32_t)slots;
    HIP_OR_FAIL(s->wf_rec.alloc(slots * (size_t)p->max_depth * (size_t)w.rec_words));
    // queue shards: a logic block appends to shard blockIdx % kWfShards, and the grid
    // (a multiple of kWfShards) deals 256-entry chunks round-robin, so a shard
    // receives at most every kWfShards-th chunk of a queue of <= slots entries
    const size_t cap = ((slots / 256) + tpt::kWfShards - 1) / tpt::kWfShards * 256;
    const size_t qn = cap * tpt::kWfShards;
    HIP_OR_FAIL(s->wf_q0.alloc(2 * qn));
    HIP_OR_FAIL(s->wf_q1.alloc(2 * qn));
    HIP_OR_FAIL(s->wf_hit.alloc(qn));
    HIP_OR_FAIL(s->wf_state.alloc(2 * qn * (size_t)w.state_words));
    HIP_OR_FAIL(s->wf_ctl.alloc(tpt::kWfCtlWords));
    HIP_OR_FAIL(s->wf_count.alloc(2 * tpt::kWfShards));
    w.shard_cap = (int32_t)cap;
    for (auto& e : s->wf_ev)
        if (!e) HIP_OR_FAIL(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    w.st0 = s->wf_state.p;
    w.st1 = s->wf_state.p + qn * (size_t)w.state_words;
    w.rec = s->wf_rec.p;
    w.q_ray0 = s->wf_q0.p;
    w.q_ray1 = s->wf_q1.p;
    w.q_hit = s->wf_hit.p;
    w.ctl = s->wf_ctl.p;
    w.refill = p->wf_refill > 0 ? p->wf_refill : 40;
    w.chunk = 128;
    w.batch = 32;
    w.logic_blocks = (int32_t)((std::min<size_t>((slots + 255) / 256, 2048) + tpt::kWfShards - 1) / tpt::kWfShards *
                               tpt::kWfShards);
    w.trace_blocks = 0;   // launch_wavefront: the CUs' occupancy
    int32_t iters = 0;
    HIP_OR_FAIL(tpt::launch_wavefront(w, s->wf_count.p, s->wf_ev, &iters, st));
    HIP_OR_FAIL(hipEventRecord(s->ev[2], st));
    HIP_OR_FAIL(hipEventSynchronize(s->ev[2]));
    float ms = 0.0f;
    HIP_OR_FAIL(hipEventElapsedTime(&ms, s->ev[1], s->ev[2]));
    trace_ms = ms;
    kernel_ms = ms;
    launches = 1 + 2 * iters;
    return TPT_OK;
}

// per-wave dump (phase-profiling builds) / traversal mismatch log (cull-verification
// builds) of a call's k_trace launches: TPT_DEBUG_WAVES names the file
struct WaveDump {
    const char* path = nullptr;
    size_t words = 0;
};

// The k_trace launches of a frame batch, as planned (launch_plan.cpp): the band
// sets fork from the scene's stream after the RNG initialisation (event ev[1]),
// run their chunks on streams of their own and join it again.  `a` holds the
// whole call (all its rows, the call's deal); list_len is its explicit deal's length.
tpt_status render_planned(tpt_scene* s, const tpt::TraceArgs& a, const tpt_params* p, const tpt::LaunchPlan& plan,
                          size_t list_len, WaveDump& dump, double& trace_ms, double& kernel_ms, int& launches,
                          int32_t* shape) {
    hipStream_t st = s->stream;
    const int nset = plan.nset;
    const size_t nf = (size_t)a.n_frames;
    const bool listed = a.band_list != nullptr;   // (an empty list has no rows for a second set)
#if defined(TPT_PROFILE_PHASES) || defined(TPT_VERIFY_CULL)
    dump.path = std::getenv("TPT_DEBUG_WAVES");
#endif
    // one record per wave of the largest grid: 8x8-pixel tiles (four lanes per
    // pixel; pair mode 16x8, one lane 16x16), 4 waves each, 8 words per wave
    const size_t dbg_launch =
        8ull * 4 * (size_t)((a.width + 7) / 8) * (size_t)((std::max(a.band_height, 1) + 7) / 8) * nf;
    dump.words = dbg_launch * std::max<size_t>(plan.launches.size(), 1);   // one region per launch
    if (dump.path) {
        HIP_OR_FAIL(s->debug.alloc(dump.words));
        HIP_OR_FAIL(hipMemsetAsync(s->debug.p, 0, dump.words * sizeof(unsigned long long), st));
    }
    HIP_OR_FAIL(s->ensure_launch_events(2 * plan.launches.size()));
    if (listed && nset > 1) {   // the sets' shares of the list, behind it
        for (int k = 0; k < nset; ++k)
            std::copy(plan.set_list[k].begin(), plan.set_list[k].end(), s->band_lists_h.begin() + plan.set_off[k]);
        HIP_OR_FAIL(hipMemcpyAsync(s->band_lists.p + list_len, s->band_lists_h.data() + list_len,
                                   list_len * sizeof(int32_t), hipMemcpyHostToDevice, st));   // (before the fork)
    }
    hipStream_t qs[tpt::kMaxPipe] = {st};
    if (nset > 1) {
        HIP_OR_FAIL(s->ensure_pipe(nset));
        HIP_OR_FAIL(hipEventRecord(s->pipe_ev[0], st));   // fork: RNG init, the sums' reset, the sets' band lists are done
        for (int k = 0; k < nset; ++k) {
            qs[k] = s->pipe[k];
            HIP_OR_FAIL(hipStreamWaitEvent(qs[k], s->pipe_ev[0], 0));
        }
    }
    // An error while the sets' launches are being queued must not leave set
    // streams writing the rng/accumulator planes behind the caller's back (the
    // next call's reset runs on the main stream): join every set before failing.
#define SET_OR_FAIL(expr)                                                                                      \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) {                                                                                \
            for (int k_ = 0; nset > 1 && k_ < nset; ++k_) (void)hipStreamSynchronize(qs[k_]);                  \
            (void)hipStreamSynchronize(st);                                                                    \
            return fail(e_ == hipErrorOutOfMemory ? TPT_ERR_OOM : TPT_ERR_HIP,                                 \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                                    \
        }                                                                                                      \
    } while (0)
    int set_chunks[tpt::kMaxPipe] = {};   // launches issued per set so far (XCD run rotation)
    for (size_t oi = 0; oi < plan.order.size(); ++oi) {
        const size_t j = plan.order[oi];
        const int k = plan.launches[j].set;
        if (plan.set_rows[k] <= 0) continue;
        tpt::TraceArgs ak = a;
        ak.samples = plan.launches[j].samples;
        ak.ahead_max = a.credit ? plan.launches[j].ahead_max : 0;   // run-ahead: what this set's later launches give
        // XCD runs: chunk c of a set rotates the runs' XCDs by c (trace.hip prologue), so a
        // set whose few rows leave the per-launch rotation incomplete still spreads its heavy
        // columns over every XCD across its chunks
        ak.xcd_rot = TPT_XCD_ROT ? (set_chunks[k]++ & 7) : 0;
        if (nset > 1) {
            ak.band_count = a.band_count * nset;
            ak.band_index = a.band_index + k * a.band_count;
            ak.band_height = plan.set_rows[k];
            if (listed) ak.band_list = s->band_lists.p + plan.set_off[k];
        }
#ifdef TPT_VERIFY_CULL
        if (dump.path) ak.debug_waves = s->debug.p;   // one log, counters[24] indexes it
#else
        if (dump.path) ak.debug_waves = s->debug.p + oi * dbg_launch;
#endif
        SET_OR_FAIL(hipEventRecord(s->lev[2 * j], qs[k]));
        SET_OR_FAIL((p->flags & TPT_FLAG_FAST) ? tpt_fast::launch_trace_ptr(&ak, qs[k], shape)
                                               : tpt::launch_trace(ak, qs[k], shape));
        SET_OR_FAIL(hipEventRecord(s->lev[2 * j + 1], qs[k]));
    }
    for (int k = 0; nset > 1 && k < nset; ++k) {   // join
        SET_OR_FAIL(hipEventRecord(s->pipe_ev[1 + k], qs[k]));
        SET_OR_FAIL(hipStreamWaitEvent(st, s->pipe_ev[1 + k], 0));
    }
    SET_OR_FAIL(hipEventRecord(s->ev[2], st));   // end of the trace phase
    SET_OR_FAIL(hipEventSynchronize(s->ev[2]));
#undef SET_OR_FAIL
    float ms = 0.0f;
    HIP_OR_FAIL(hipEventElapsedTime(&ms, s->ev[1], s->ev[2]));
    trace_ms = ms;   // wall time of the trace phase (overlapping launches counted once)
    for (size_t j = 0; j < plan.launches.size(); ++j) {
        if (plan.set_rows[plan.launches[j].set] <= 0) continue;
        HIP_OR_FAIL(hipEventElapsedTime(&ms, s->lev[2 * j], s->lev[2 * j + 1]));
        kernel_ms += ms;
        ++launches;
    }
    return TPT_OK;
}

}  // namespace

extern "C" {

tpt_status tpt_render(tpt_scene* s, const tpt_env* env, const tpt_camera* cam, const tpt_params* p,
                      float* radiance_out, uint8_t* bgra_out, tpt_stats* stats) {
    if (!p) return fail(TPT_ERR_INVALID_ARG, "null argument");
    const uint64_t seed = p->seed;
    return tpt_render_frames(s, env, cam, p, 1, &seed, &radiance_out, &bgra_out, stats);
}

tpt_status tpt_render_frames(tpt_scene* s, const tpt_env* env, const tpt_camera* cam, const tpt_params* p,
                             int32_t n_frames, const uint64_t* seeds, float* const* radiance_outs,
                             uint8_t* const* bgra_outs, tpt_stats* stats) {
    auto t_start = std::chrono::steady_clock::now();
    if (!s || !cam || !p || !seeds) return fail(TPT_ERR_INVALID_ARG, "null argument");
    if (n_frames < 1 || n_frames > 65535) return fail(TPT_ERR_INVALID_ARG, "bad frame count");
    if (!s->built) return fail(TPT_ERR_INVALID_ARG, "scene not built (call tpt_scene_build)");
    if (p->width <= 0 || p->height <= 0 || p->spp <= 0 || p->max_depth < 1 || p->max_depth > 64)
        return fail(TPT_ERR_INVALID_ARG, "bad frame parameters");
    if ((int64_t)p->width * p->height > (int64_t)1 << 30) return fail(TPT_ERR_INVALID_ARG, "frame too large");
    const int band_rows = p->band_rows > 0 ? p->band_rows : 16;
    // an explicit deal (band_list) replaces the interleaved one (band_count, band_index)
    const bool listed = p->band_list != nullptr;
    const int band_count = listed ? 1 : (p->band_count > 0 ? p->band_count : 1);
    const int band_index = listed ? 0 : p->band_index;
    if (!listed && (p->band_index < 0 || p->band_index >= band_count))
        return fail(TPT_ERR_INVALID_ARG, "bad band index");
    if (env && env->device != s->device) return fail(TPT_ERR_INVALID_ARG, "env lives on another device");
    const int W = p->width, H = p->height;
    const int n_bands = (H + band_rows - 1) / band_rows;
    std::vector<int32_t> list;
    if (listed) {
        if (p->band_list_len < 0 || p->band_list_len > n_bands)
            return fail(TPT_ERR_INVALID_ARG, "band_list_len: 0 .. ceil(height / band_rows)");
        list.assign(p->band_list, p->band_list + p->band_list_len);
        std::vector<uint8_t> seen((size_t)n_bands, 0);
        const bool partial = H % band_rows != 0;   // the last band is short: it must come last (kernels
        for (size_t i = 0; i < list.size(); ++i) {  // map local row ly to list[ly / band_rows])
            if (list[i] < 0 || list[i] >= n_bands || seen[(size_t)list[i]]++ ||
                (partial && list[i] == n_bands - 1 && i + 1 != list.size()))
                return fail(TPT_ERR_INVALID_ARG, "band_list: distinct band ids below ceil(height / band_rows), "
                                                 "a short last band last");
        }
    }
    DeviceGuard g(s->device);
    hipStream_t st = s->stream;
    const size_t npix = (size_t)W * (size_t)H;
    const size_t nf = (size_t)n_frames;
    const int bh = listed ? tpt::band_list_rows(list.data(), list.size(), band_rows, H)
                          : tpt::band_height_of(H, band_rows, band_count, band_index);
    const std::vector<uint64_t> fseeds(seeds, seeds + nf);

    const bool resume = (p->flags & TPT_FLAG_ACCUMULATE) && s->acc_valid && s->acc_w == W && s->acc_h == H &&
                        s->acc_rows == band_rows && s->acc_count == band_count && s->acc_index == band_index &&
                        s->acc_list == list && s->acc_seeds == fseeds && s->rng.n == 6 * npix * nf &&
                        s->accum.n == 3 * npix * nf;
    s->acc_valid = false;   // re-armed once this call has completed
    // per-frame state planes, frame f at offset f * (6|3) * npix
    HIP_OR_FAIL(s->rng.alloc(6 * npix * nf));
    HIP_OR_FAIL(s->accum.alloc(3 * npix * nf));
    HIP_OR_FAIL(s->credit.alloc(npix * nf));
    HIP_OR_FAIL(s->counters.alloc(32));
    if (!resume) HIP_OR_FAIL(hipMemsetAsync(s->accum.p, 0, 3 * npix * nf * sizeof(float), st));   // thrust::fill (:534)
    HIP_OR_FAIL(hipMemsetAsync(s->counters.p, 0, 32 * sizeof(unsigned long long), st));
    // the explicit deal's list on the device: the whole list first, the band sets'
    // shares after it (written once the launch plan is known: render_planned)
    const int32_t* d_list = nullptr;
    if (listed && !list.empty()) {
        s->band_lists_h.assign(2 * list.size(), 0);
        std::copy(list.begin(), list.end(), s->band_lists_h.begin());
        HIP_OR_FAIL(s->band_lists.alloc(std::max(s->band_lists.n, 2 * list.size())));
        HIP_OR_FAIL(hipMemcpyAsync(s->band_lists.p, s->band_lists_h.data(), list.size() * sizeof(int32_t),
                                   hipMemcpyHostToDevice, st));
        d_list = s->band_lists.p;
    }
    if (p->band_cost) {
        HIP_OR_FAIL(s->band_cost.alloc(std::max<size_t>(s->band_cost.n, (size_t)n_bands)));
        HIP_OR_FAIL(hipMemsetAsync(s->band_cost.p, 0, (size_t)n_bands * sizeof(unsigned long long), st));
    }

    // setupRandSeed (:513), one seed per frame; a progressive call continues the persisted streams
    HIP_OR_FAIL(hipEventRecord(s->ev[0], st));
    if (bh > 0 && !resume)
        for (size_t f = 0; f < nf; ++f)
            HIP_OR_FAIL(tpt::launch_rng_init(s->jumps.p, fseeds[f], W, band_rows, band_count, band_index, d_list, bh,
                                             H, s->rng.p + f * 6 * npix, st));
    HIP_OR_FAIL(hipEventRecord(s->ev[1], st));
    // an asynchronous scene build's host half ran while the above was enqueued
    double tree_wait_ms = 0.0;
    {
        const tpt_status bs = finish_pending(s, &tree_wait_ms);
        if (bs != TPT_OK) return bs;
    }
    const uint64_t total_spp = (resume ? s->acc_spp : 0) + (uint64_t)p->spp;
    if (total_spp > (uint64_t)INT32_MAX) return fail(TPT_ERR_INVALID_ARG, "accumulated spp overflow");

    tpt::TraceArgs a{};
    fill_trace_args(s, env, cam, a);
    a.inv_w = 1.0f / (float)W;
    a.inv_h = 1.0f / (float)H;
    a.width = W;
    a.height = H;
    a.band_rows = band_rows;
    a.band_count = band_count;
    a.band_index = band_index;
    a.band_list = d_list;
    a.band_cost = p->band_cost ? s->band_cost.p : nullptr;
    a.band_height = bh;
    a.n_frames = n_frames;
    a.max_depth = p->max_depth;
    a.flags = p->flags;
    // culls without the exactness guards (trace.hip "Culling"); the tolerance mode too:
    // its C5 band measures the same with the guards kept
    if (p->flags & (TPT_FLAG_APPROX_CULL | TPT_FLAG_FAST)) {
        a.cull_eps = 0.0f;
        a.n_sliver_groups = 0;
        a.graze = 0;
    }
    // A15 env next-event estimation: opt-in, needs an env with a non-empty distribution
    a.env_is = ((p->flags & TPT_FLAG_ENV_IS) && env && env->is_total > 0.0f) ? 1 : 0;
    a.rng = s->rng.p;
    a.accum = s->accum.p;
    a.counters = s->counters.p;
    a.debug_waves = nullptr;

    // how to launch: the lane mode, the kernel's batching, the schedule (launch_plan.cpp)
    tpt::PlanInput pin;
    pin.width = W;
    pin.band_rows = band_rows;
    pin.bh = bh;
    pin.height = H;
    pin.n_frames = n_frames;
    pin.band_count = band_count;
    pin.band_index = band_index;
    pin.listed = listed;
    pin.list = list.data();
    pin.list_len = list.size();
    pin.spp = p->spp;
    pin.flags = p->flags;
    pin.lanes_per_pixel = p->lanes_per_pixel;
    pin.refill = p->refill;
    pin.leaf_batch = p->leaf_batch;
    pin.spp_per_launch = p->spp_per_launch;
    pin.pipe_sets = p->pipe_sets;
    pin.pipe_chunks = p->pipe_chunks;
    pin.n_faces = s->n_faces;
    pin.n_lights = s->n_lights;
    pin.n_materials = s->n_materials;
    pin.resident_lanes = s->resident_lanes;
    pin.env_is = a.env_is != 0;
    pin.quad_fits = tpt::trace_quad_fits(a);
    pin.max_depth = p->max_depth;
    pin.any_emitter = s->any_emitter != 0;
    const tpt::LaunchPlan plan = tpt::plan_launches(pin);
    if (plan.status != TPT_OK) return fail(plan.status, plan.message);
    a.pair = plan.pair ? 1 : 0;
    a.quad = plan.quad ? 1 : 0;
    a.refill = plan.refill;
    a.drained = plan.drained ? 1 : 0;
    a.leaf_kb = plan.leaf_kb;
    a.xcd_run = plan.xcd_run;
    a.xcd_rot = 0;   // (per launch: render_planned)
    // Run-ahead (trace_variant.hpp trace_runs_ahead): on when the variant these launches select is
    // compiled with it and some set's spp is cut into several launches (the default pipeline, forced
    // pipe_sets / pipe_chunks, an explicit spp_per_launch).  The sets render disjoint rows and a set's
    // launches are stream-ordered, so the plane needs no atomics.  A set's last launch has ahead_max 0
    // and leaves every pixel's credit at zero, so the plane is zero again at the end of the call and a
    // TPT_FLAG_ACCUMULATE continuation starts from zero; it is zeroed here all the same, on the main
    // stream, before render_planned forks to the sets' streams.
    // band_cost with run-ahead: a band's cost moves between a set's launches, its sum over the call
    // (what the caller reads) covers the same samples.
    a.ahead_max = 0;   // (per launch: render_planned)
    a.credit = nullptr;
    bool chunked = false;
    for (const tpt::PlanLaunch& l : plan.launches) chunked = chunked || l.ahead_max > 0;
    bool ahead = chunked && !(p->flags & TPT_FLAG_WAVEFRONT) && tpt::trace_args_run_ahead(a);
#ifdef TPT_PROFILE_PHASES
    if (std::getenv("TPT_DEBUG_NO_AHEAD")) ahead = false;   // the lane-step split without it from the same build
#endif
    if (ahead && bh > 0) {
        HIP_OR_FAIL(hipMemsetAsync(s->credit.p, 0, npix * nf * sizeof(int32_t), st));
        a.credit = s->credit.p;
    }

    double trace_ms = 0.0, kernel_ms = 0.0;
    int launches = 0;
    WaveDump dump;
    int32_t shape[tpt::kTraceShapeWords] = {};   // (all zero: the wavefront variant)
    if ((p->flags & TPT_FLAG_WAVEFRONT) && (p->flags & (TPT_FLAG_FAST | TPT_FLAG_APPROX_CULL)))
        return fail(TPT_ERR_INVALID_ARG, "TPT_FLAG_WAVEFRONT runs the exact traversal only");
    const tpt_status ts = (p->flags & TPT_FLAG_WAVEFRONT)
                              ? render_wavefront(s, a, p, n_frames, bh, trace_ms, kernel_ms, launches)
                              : render_planned(s, a, p, plan, list.size(), dump, trace_ms, kernel_ms, launches, shape);
    if (ts != TPT_OK) return ts;
    if (std::getenv("TPT_DEBUG_SHAPE"))   // the k_trace workgroups this call ran, and the runtime's residency answer
        std::fprintf(stderr,
                     "tpt trace shape: wg_waves %d resident_blocks %d need_blocks %d lds_bytes %d stack_slots %d "
                     "rec_levels %d\n",
                     shape[0], shape[1], shape[2], shape[3], shape[4], shape[5]);

    // copyToFB (:553) + radiance readout, per frame
    HIP_OR_FAIL(hipEventRecord(s->ev[2], st));
    Staging sg(st);
    for (size_t f = 0; f < nf; ++f) {
        tpt::ResolveArgs r{};
        r.accum = s->accum.p + f * 3 * npix;
        r.width = W;
        r.height = H;
        r.band_rows = band_rows;
        r.band_count = band_count;
        r.band_index = band_index;
        r.band_list = d_list;
        r.band_height = bh;
        r.spp = (int)total_spp;
        // the caller's bytes go up first: the resolve writes only the call's rows, and no alpha
        HIP_OR_FAIL(sg.inout(s->radiance_tmp, radiance_outs ? radiance_outs[f] : nullptr, 3 * npix, &r.radiance));
        HIP_OR_FAIL(sg.inout(s->bgra_tmp, bgra_outs ? bgra_outs[f] : nullptr, 4 * npix, &r.bgra));
        if (bh > 0 && (r.radiance || r.bgra)) HIP_OR_FAIL(tpt::launch_resolve(r, st));
        // host outputs share one staging buffer: copy back before the next frame reuses it
        HIP_OR_FAIL(sg.finish());
    }
    HIP_OR_FAIL(hipEventRecord(s->ev[3], st));
    unsigned long long cnt[32] = {0};
    HIP_OR_FAIL(hipMemcpyAsync(cnt, s->counters.p, sizeof cnt, hipMemcpyDeviceToHost, st));
    HIP_OR_FAIL(hipStreamSynchronize(st));
    if (cnt[4] != 0) return fail(TPT_ERR_HIP, "traversal stack overflow (BVH deeper than sized)");
    if (p->band_cost) {   // per band this call rendered: its waves' summed life, in microseconds
        s->band_cost_h.resize((size_t)n_bands);
        HIP_OR_FAIL(hipMemcpy(s->band_cost_h.data(), s->band_cost.p, (size_t)n_bands * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost));
        for (int b = 0; b < n_bands; ++b) {
            const bool mine = listed ? std::find(list.begin(), list.end(), b) != list.end()
                                     : b % band_count == band_index;
            if (mine) p->band_cost[b] = (float)((double)s->band_cost_h[(size_t)b] / 100.0);   // 100-MHz ticks
        }
    }
    if (dump.path) {
#ifdef TPT_VERIFY_CULL
        const size_t dump_words = std::min<size_t>(dump.words, 16 * std::min<unsigned long long>(cnt[24], 4096));
#else
        const size_t dump_words = dump.words;
#endif
        std::vector<unsigned long long> h(dump_words);
        if (dump_words)
            HIP_OR_FAIL(hipMemcpy(h.data(), s->debug.p, dump_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen(dump.path, "wb")) {
            std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
            std::fclose(f);
        }
    }
#if defined(TPT_PROFILE_PHASES) || defined(TPT_VERIFY_CULL)
    if (std::getenv("TPT_DEBUG_COUNTERS")) {   // raw kernel counters (TPT_PROFILE_PHASES builds: 6..15 phases, 16..22 shading-pass sections, 29..31 the unwind)
        std::fprintf(stderr, "tpt counters:");
        for (int i = 0; i < 32; ++i) std::fprintf(stderr, " %llu", cnt[i]);
        std::fprintf(stderr, "\n");
    }
#endif
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->traversals = cnt[0];
        stats->internal_visits = cnt[1];
        stats->wide_visits = cnt[5];
        stats->local_rays = cnt[9];
        stats->accumulated_spp = total_spp;
        stats->leaf_tests = cnt[2];
        stats->shade_hits = cnt[3];
        stats->pixels = (uint64_t)W * (uint64_t)bh * (uint64_t)nf;
        stats->samples = stats->pixels * (uint64_t)p->spp;
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, s->ev[0], s->ev[1]);
        stats->rng_init_ms = ms;
        stats->trace_ms = trace_ms;
        stats->trace_kernel_ms = kernel_ms;
        stats->tree_wait_ms = tree_wait_ms;
        (void)hipEventElapsedTime(&ms, s->ev[2], s->ev[3]);
        stats->resolve_ms = ms;
        stats->trace_launches = launches;
        stats->wg_waves = shape[0];
        stats->resident_lanes = s->resident_lanes;
        stats->lanes_per_pixel = plan.quad ? 4 : (plan.pair_kernel ? 2 : 1);
        stats->drained = a.drained;
        stats->total_ms =
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    // the persisted streams and sums now belong to this batch: a following
    // TPT_FLAG_ACCUMULATE call with the same frames continues them
    s->acc_valid = true;
    s->acc_w = W;
    s->acc_h = H;
    s->acc_rows = band_rows;
    s->acc_count = band_count;
    s->acc_index = band_index;
    s->acc_list = list;
    s->acc_seeds = fseeds;
    s->acc_spp = total_spp;
    return TPT_OK;
}

}  // extern "C"
