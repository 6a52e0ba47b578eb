// api_post.cpp -- the post-pass entry points of the C-ABI (post.hip): tpt_render_aov, tpt_render_aov_path,
// tpt_render_aov_path_points, tpt_denoise, tpt_history_* (tpt_history_set_clip too), tpt_temporal, tpt_temporal_motion, tpt_temporal_path,
// tpt_temporal_deform, tpt_denoise_svgf and tpt_upsample, and of tonemap.hip: tpt_exposure_* and
// tpt_tonemap.  Each takes its buffers from either
// side: host buffers go through the device staging the scene / history keeps
// (api_internal.hpp Staging).
#include <cmath>

#include "api_internal.hpp"

namespace {

// Inverse of a column-major 4x4 matrix by Gauss-Jordan elimination with partial
// pivoting in double, rounded to float.  false: singular.
bool invert4(const float* m, float* out) {
    double a[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            a[i][j] = (double)m[4 * j + i];
            a[i][4 + j] = i == j ? 1.0 : 0.0;
        }
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        for (int r = c + 1; r < 4; ++r)
            if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
        if (!(std::fabs(a[piv][c]) > 0.0)) return false;
        if (piv != c)
            for (int j = 0; j < 8; ++j) std::swap(a[c][j], a[piv][j]);
        const double d = 1.0 / a[c][c];
        for (int j = 0; j < 8; ++j) a[c][j] *= d;
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double f = a[r][c];
            if (f != 0.0)
                for (int j = 0; j < 8; ++j) a[r][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) out[4 * j + i] = (float)a[i][4 + j];
    return true;
}

// The time between two events of a stream that has run, as the stats structs hold it.
hipError_t elapsed_ms(hipEvent_t e0, hipEvent_t e1, double* out) {
    float ms = 0.0f;
    const hipError_t e = hipEventElapsedTime(&ms, e0, e1);
    if (e == hipSuccess) *out = ms;
    return e;
}

// The scene, the camera and the whole frame as the feature-buffer kernels take them.
tpt::TraceArgs frame_trace_args(tpt_scene* s, const tpt_camera* cam, int32_t W, int32_t H) {
    tpt::TraceArgs a{};
    fill_trace_args(s, nullptr, cam, a);
    a.width = W;
    a.height = H;
    a.inv_w = 1.0f / (float)W;
    a.inv_h = 1.0f / (float)H;
    return a;
}

// The five feature planes of `out` as the kernels' outputs: host ones through the scene's staging.
hipError_t stage_aov(Staging& sg, tpt_scene* s, const tpt_aov* out, size_t npix, tpt::AovArgs& o) {
    hipError_t e = sg.out(s->aov_f3[0], out->albedo, 3 * npix, &o.albedo);
    if (e == hipSuccess) e = sg.out(s->aov_i[0], out->face, npix, &o.face);
    if (e == hipSuccess) e = sg.out(s->aov_f3[1], out->normal, 3 * npix, &o.normal);
    if (e == hipSuccess) e = sg.out(s->aov_i[1], out->material, npix, &o.material);
    if (e == hipSuccess) e = sg.out(s->aov_depth, out->depth, npix, &o.depth);
    return e;
}

// What both a-trous filters make of their parameters: 1 / sigma^2 kept finite, sigma_z^2, and
// whether steps 1 and 2 go through the LDS kernels.
float inv_sq(double sigma) { return (float)std::min(1.0 / (sigma * sigma), 3.402823466e+38); }
struct FilterConsts {
    float inv_sn2, sz2;
    bool use_lds;
};
FilterConsts filter_consts(float sigma_normal, float sigma_depth, bool direct) {
    return {inv_sq(sigma_normal), (float)((double)sigma_depth * sigma_depth), !direct};
}

}  // namespace

extern "C" {

// First-hit feature buffers (post.hip k_aov): the whole frame, one ray per pixel
// centre.  Host outputs are written to the scene's staging buffers and copied back.
tpt_status tpt_render_aov(tpt_scene* s, const tpt_camera* cam, int32_t W, int32_t H, const tpt_aov* out,
                          double* trace_ms) {
    if (!s || !s->built) return fail(TPT_ERR_INVALID_ARG, "scene not built");
    if (!cam || !out) return fail(TPT_ERR_INVALID_ARG, "null argument");
    if (W <= 0 || H <= 0) return fail(TPT_ERR_INVALID_ARG, "bad frame size");
    if (!out->albedo && !out->normal && !out->depth && !out->face && !out->material)
        return fail(TPT_ERR_INVALID_ARG, "no feature buffer requested: every pointer of out is null");
    {
        const tpt_status bs = finish_pending(s);
        if (bs != TPT_OK) return bs;
    }
    DeviceGuard g(s->device);
    hipStream_t st = s->stream;
    const size_t npix = (size_t)W * (size_t)H;
    const tpt::TraceArgs a = frame_trace_args(s, cam, W, H);
    tpt::AovArgs o{};
    Staging sg(st);
    HIP_OR_FAIL(stage_aov(sg, s, out, npix, o));
    HIP_OR_FAIL(hipEventRecord(s->ev[0], st));
    HIP_OR_FAIL(tpt::launch_aov(a, o, st));
    HIP_OR_FAIL(hipEventRecord(s->ev[1], st));
    HIP_OR_FAIL(sg.finish());
    HIP_OR_FAIL(hipStreamSynchronize(st));
    if (trace_ms) HIP_OR_FAIL(elapsed_ms(s->ev[0], s->ev[1], trace_ms));
    return TPT_OK;
}

// Mirror-path feature buffers (post.hip k_aov_path; DESIGN.md section 5 "Post-pass"):
// tpt_render_aov's call with the bounce counts as a sixth output and two statistics,
// counted by the kernel in the spread counters and reduced here.  With points_out
// (tpt_render_aov_path_points) the sibling kernel k_aov_path_points runs instead.
static tpt_status aov_path_pass(tpt_scene* s, const tpt_camera* cam, int32_t W, int32_t H,
                                const tpt_aov_path_params* p, const tpt_aov* out, int32_t* bounces_out,
                                float* points_out, tpt_aov_path_stats* stats) {
    if (!s || !s->built) return fail(TPT_ERR_INVALID_ARG, "scene not built");
    if (!cam) return fail(TPT_ERR_INVALID_ARG, "null camera");
    if (!p) return fail(TPT_ERR_INVALID_ARG, "null params");
    if (W <= 0 || H <= 0) return fail(TPT_ERR_INVALID_ARG, "bad frame size");
    if (p->max_bounces < 0 || p->max_bounces > 64) return fail(TPT_ERR_INVALID_ARG, "max_bounces must be 0..64");
    if (p->flags != 0) return fail(TPT_ERR_INVALID_ARG, "unknown aov path flags");
    if (!bounces_out && !points_out && !(out && (out->albedo || out->normal || out->depth || out->face || out->material)))
        return fail(TPT_ERR_INVALID_ARG,
                    "no feature buffer requested: every pointer of out and bounces_out are null");
    {
        const tpt_status bs = finish_pending(s);
        if (bs != TPT_OK) return bs;
    }
    DeviceGuard g(s->device);
    hipStream_t st = s->stream;
    const size_t npix = (size_t)W * (size_t)H;
    const tpt::TraceArgs a = frame_trace_args(s, cam, W, H);
    const tpt_aov none{};
    tpt::AovArgs o{};
    tpt::AovPathArgs pa{};
    pa.max_bounces = p->max_bounces;
    HIP_OR_FAIL(s->ap_count.alloc(2));
    pa.followed = s->ap_count.set(0);
    pa.deepest = s->ap_count.set(1);
    Staging sg(st);
    HIP_OR_FAIL(stage_aov(sg, s, out ? out : &none, npix, o));
    HIP_OR_FAIL(sg.out(s->ap_bounces, bounces_out, npix, &pa.bounces));
    float* points = nullptr;
    HIP_OR_FAIL(sg.out(s->ap_points, points_out, 3 * npix, &points));
    HIP_OR_FAIL(s->ap_count.zero(st));
    HIP_OR_FAIL(hipEventRecord(s->ev[0], st));
    HIP_OR_FAIL(points ? tpt::launch_aov_path_points(a, o, pa, points, st) : tpt::launch_aov_path(a, o, pa, st));
    HIP_OR_FAIL(hipEventRecord(s->ev[1], st));
    HIP_OR_FAIL(sg.finish());
    HIP_OR_FAIL(s->ap_count.fetch(st));
    HIP_OR_FAIL(hipStreamSynchronize(st));
    if (stats) {
        HIP_OR_FAIL(elapsed_ms(s->ev[0], s->ev[1], &stats->trace_ms));
        stats->followed = s->ap_count.sum(0);
        stats->deepest = (int32_t)s->ap_count.max(1);
    }
    return TPT_OK;
}

tpt_status tpt_render_aov_path(tpt_scene* s, const tpt_camera* cam, int32_t W, int32_t H,
                               const tpt_aov_path_params* p, const tpt_aov* out, int32_t* bounces_out,
                               tpt_aov_path_stats* stats) {
    return aov_path_pass(s, cam, W, H, p, out, bounces_out, nullptr, stats);
}

tpt_status tpt_render_aov_path_points(tpt_scene* s, const tpt_camera* cam, int32_t W, int32_t H,
                                      const tpt_aov_path_params* p, const tpt_aov* out, int32_t* bounces_out,
                                      float* points_out, tpt_aov_path_stats* stats) {
    return aov_path_pass(s, cam, W, H, p, out, bounces_out, points_out, stats);
}

// The a-trous denoiser (post.hip; DESIGN.md section 5 "Post-pass"): pack, one launch
// per iteration between the two colour planes, resolve.  Host inputs are uploaded
// to the scene's staging buffers, host outputs copied back from them.
tpt_status tpt_denoise(tpt_scene* s, int32_t W, int32_t H, const float* radiance_in, const tpt_aov* guides,
                       const tpt_denoise_params* p, float* radiance_out, uint8_t* bgra_out,
                       tpt_denoise_stats* stats) {
    if (!s) return fail(TPT_ERR_INVALID_ARG, "null scene");
    if (!radiance_in || !guides || !p) return fail(TPT_ERR_INVALID_ARG, "null argument");
    if (!guides->albedo || !guides->normal || !guides->depth)
        return fail(TPT_ERR_INVALID_ARG, "the denoiser needs the albedo, normal and depth guides");
    if (W <= 0 || H <= 0) return fail(TPT_ERR_INVALID_ARG, "bad frame size");
    if (p->iterations < 0 || p->iterations > 8) return fail(TPT_ERR_INVALID_ARG, "iterations must be 0..8");
    if (!(p->sigma_color > 0.0f) || !(p->sigma_normal > 0.0f) || !(p->sigma_depth > 0.0f))
        return fail(TPT_ERR_INVALID_ARG, "sigma_color, sigma_normal and sigma_depth must be > 0");
    if (p->flags & ~(TPT_DENOISE_DEMODULATE | TPT_DENOISE_DIRECT)) return fail(TPT_ERR_INVALID_ARG, "unknown denoise flags");
    if (!radiance_out && !bgra_out) return fail(TPT_ERR_INVALID_ARG, "no output buffer");
    DeviceGuard g(s->device);
    hipStream_t st = s->stream;
    const size_t npix = (size_t)W * (size_t)H;
    // iterations 0: the input bit for bit, so no demodulation round trip
    const bool demod = (p->flags & TPT_DENOISE_DEMODULATE) && p->iterations > 0;
    HIP_OR_FAIL(s->dn_color[0].alloc(npix));
    HIP_OR_FAIL(s->dn_color[1].alloc(npix));
    HIP_OR_FAIL(s->dn_guide.alloc(npix));
    tpt::DenoiseArgs d{};
    d.npix = npix;
    d.width = W;
    d.height = H;
    d.demodulate = demod ? 1 : 0;
    d.color0 = s->dn_color[0].p;
    d.guide = s->dn_guide.p;
    Staging sg(st);
    HIP_OR_FAIL(sg.in(s->dn_rad, radiance_in, 3 * npix, &d.radiance_in));
    HIP_OR_FAIL(sg.in(s->dn_f3[0], guides->albedo, 3 * npix, &d.albedo));
    HIP_OR_FAIL(sg.in(s->dn_f3[1], guides->normal, 3 * npix, &d.normal));
    HIP_OR_FAIL(sg.in(s->dn_depth, guides->depth, npix, &d.depth));
    // radiance in and out share dn_rad: pack has read it by the time resolve writes it
    HIP_OR_FAIL(sg.out(s->dn_rad, radiance_out, 3 * npix, &d.radiance_out));
    // alpha is untouched: the caller's bytes go up first
    HIP_OR_FAIL(sg.inout(s->dn_bgra, bgra_out, 4 * npix, &d.bgra));
    HIP_OR_FAIL(hipEventRecord(s->ev[0], st));
    HIP_OR_FAIL(tpt::launch_denoise_pack(d, st));
    HIP_OR_FAIL(hipEventRecord(s->ev[1], st));
    tpt::AtrousArgs f{};
    f.guide = s->dn_guide.p;
    f.width = W;
    f.height = H;
    const FilterConsts fc = filter_consts(p->sigma_normal, p->sigma_depth, p->flags & TPT_DENOISE_DIRECT);
    f.inv_sn2 = fc.inv_sn2;
    f.sz2 = fc.sz2;
    for (int i = 0; i < p->iterations; ++i) {
        f.src = s->dn_color[i & 1].p;
        f.dst = s->dn_color[(i + 1) & 1].p;
        f.step = 1 << i;
        f.inv_sc2 = inv_sq((double)p->sigma_color / (double)(1 << i));   // sigma_c,i = sigma_color 2^-i
        HIP_OR_FAIL(tpt::launch_atrous(f, fc.use_lds, st));
    }
    HIP_OR_FAIL(hipEventRecord(s->ev[2], st));
    d.color0 = s->dn_color[p->iterations & 1].p;
    HIP_OR_FAIL(tpt::launch_denoise_resolve(d, st));
    HIP_OR_FAIL(hipEventRecord(s->ev[3], st));
    HIP_OR_FAIL(sg.finish());
    HIP_OR_FAIL(hipStreamSynchronize(st));
    if (stats) {
        HIP_OR_FAIL(elapsed_ms(s->ev[0], s->ev[1], &stats->pack_ms));
        HIP_OR_FAIL(elapsed_ms(s->ev[1], s->ev[2], &stats->filter_ms));
        HIP_OR_FAIL(elapsed_ms(s->ev[2], s->ev[3], &stats->resolve_ms));
    }
    return TPT_OK;
}

// Temporal reprojection and accumulation (post.hip k_temporal; DESIGN.md section 5
// "Post-pass").  The handle keeps the two sets of state planes, the previous call's
// camera and the device staging of host buffers.
tpt_status tpt_history_create(tpt_scene* s, int32_t W, int32_t H, tpt_history** out) {
    if (!s) return fail(TPT_ERR_INVALID_ARG, "null scene");
    if (!out) return fail(TPT_ERR_INVALID_ARG, "null out");
    if (W <= 0 || H <= 0) return fail(TPT_ERR_INVALID_ARG, "bad frame size");
    DeviceGuard g(s->device);
    std::unique_ptr<tpt_history> h(new tpt_history);
    h->scene = s;
    h->device = s->device;
    h->width = W;
    h->height = H;
    const size_t npix = (size_t)W * (size_t)H;
    for (auto& set : h->state)
        for (auto& plane : set) HIP_OR_FAIL(plane.alloc(npix));
    HIP_OR_FAIL(h->count.alloc(1));
    {   // tpt_temporal_motion: which object each face belongs to, and room for the objects' records
        std::vector<int32_t> fo((size_t)s->n_faces);
        for (int32_t o = 0; o < s->n_objects; ++o) {
            const int32_t end = o + 1 < s->n_objects ? s->h_lut_begin[o + 1] : s->n_faces;
            for (int32_t f = std::max(s->h_lut_begin[o], 0); f < std::min(end, s->n_faces); ++f) fo[f] = o;
        }
        HIP_OR_FAIL(h->face_object.upload(fo.data(), fo.size(), s->stream));
        HIP_OR_FAIL(hipStreamSynchronize(s->stream));   // (fo is freed below)
        HIP_OR_FAIL(h->records.alloc((size_t)s->n_objects * tpt::kMotionRecordFloats));
        HIP_OR_FAIL(h->h_records.alloc((size_t)s->n_objects * tpt::kMotionRecordFloats));
    }
    for (auto& e : h->ev) HIP_OR_FAIL(hipEventCreate(&e));
    for (auto& e : h->clip_ev) HIP_OR_FAIL(hipEventCreate(&e));
    *out = h.release();
    return TPT_OK;
}

tpt_status tpt_history_reset(tpt_history* h) {
    if (!h) return fail(TPT_ERR_INVALID_ARG, "null history");
    h->valid = false;
    h->prev_vert_trans.clear();
    ++h->serial;   // tpt_temporal_deform's snapshot is no longer the previous call's
    return TPT_OK;
}

void tpt_history_destroy(tpt_history* h) { delete h; }

// History clipping (post.hip k_clip_box and k_temporal with ClipArgs; DESIGN.md section 5
// "History clipping"): a setting of the history that every temporal entry point obeys.
tpt_status tpt_history_set_clip(tpt_history* h, const tpt_clip_params* p) {
    if (!h) return fail(TPT_ERR_INVALID_ARG, "null history");
    if (!p) {
        h->clip_on = false;
        return TPT_OK;
    }
    if (p->radius < 1 || p->radius > 3) return fail(TPT_ERR_INVALID_ARG, "clip radius must be 1..3");
    if (!(std::isfinite(p->gamma) && p->gamma > 0.0f)) return fail(TPT_ERR_INVALID_ARG, "clip gamma must be finite and > 0");
    if (p->max_history < 1 || p->max_history > 65536)
        return fail(TPT_ERR_INVALID_ARG, "clip max_history must be 1..65536");
    if (p->flags != 0) return fail(TPT_ERR_INVALID_ARG, "unknown clip flags");
    h->clip = *p;
    h->clip_on = true;
    return TPT_OK;
}

tpt_status tpt_history_clip_stats(const tpt_history* h, tpt_clip_stats* out) {
    if (!h) return fail(TPT_ERR_INVALID_ARG, "null history");
    if (!out) return fail(TPT_ERR_INVALID_ARG, "null out");
    *out = h->clip_stats;
    return TPT_OK;
}

// What tpt_temporal_path passes on top of tpt_temporal's arguments.
struct PathInputs {
    const int32_t* bounces;
    const float* points;
    float point_tol;
};

// The four temporal entry points.  Plain and Path: face guide and motion_out unused; path: not null
// for Path alone.
static tpt_status temporal_pass(tpt_history* h, const tpt_camera* cam, const float* radiance_in,
                                const tpt_aov* guides, const tpt_temporal_params* p, float* radiance_out,
                                float* variance_out, float* history_len_out, float* motion_out, uint8_t* bgra_out,
                                tpt_temporal_stats* stats, TemporalKind kind, const PathInputs* path = nullptr) {
    const bool motion = kind == TemporalKind::Motion, deform = kind == TemporalKind::Deform;
    if (!h) return fail(TPT_ERR_INVALID_ARG, "null history");
    if (!cam) return fail(TPT_ERR_INVALID_ARG, "null camera");
    if (!radiance_in) return fail(TPT_ERR_INVALID_ARG, "null radiance_in");
    if (!guides) return fail(TPT_ERR_INVALID_ARG, "null guides");
    if (!p) return fail(TPT_ERR_INVALID_ARG, "null params");
    if (p->flags & ~(TPT_TEMPORAL_DEMODULATE | TPT_TEMPORAL_TILES)) return fail(TPT_ERR_INVALID_ARG, "unknown temporal flags");
    const bool demod = (p->flags & TPT_TEMPORAL_DEMODULATE) != 0;
    if (!guides->normal || !guides->depth || !guides->material)
        return fail(TPT_ERR_INVALID_ARG, "temporal accumulation needs the normal, depth and material guides");
    if (motion && !guides->face)
        return fail(TPT_ERR_INVALID_ARG, "motion-aware accumulation needs the face guides too");
    if (deform && !guides->face)
        return fail(TPT_ERR_INVALID_ARG, "accumulation on deforming meshes needs the face guides too");
    if (demod && !guides->albedo)
        return fail(TPT_ERR_INVALID_ARG, "TPT_TEMPORAL_DEMODULATE needs the albedo guides");
    if (!(p->alpha > 0.0f && p->alpha <= 1.0f)) return fail(TPT_ERR_INVALID_ARG, "alpha must be in (0, 1]");
    if (!(p->depth_tol > 0.0f)) return fail(TPT_ERR_INVALID_ARG, "depth_tol must be > 0");
    if (!(p->normal_min >= -1.0f && p->normal_min <= 1.0f))
        return fail(TPT_ERR_INVALID_ARG, "normal_min must be in [-1, 1]");
    if (p->max_history < 1 || p->max_history > 65536) return fail(TPT_ERR_INVALID_ARG, "max_history must be 1..65536");
    if (!radiance_out && !bgra_out) return fail(TPT_ERR_INVALID_ARG, "no output buffer: radiance_out and bgra_out are null");
    if (path && (!path->bounces || !path->points))
        return fail(TPT_ERR_INVALID_ARG, "accumulation through mirrors needs the bounce counts and the terminal points");
    if (path && !(path->point_tol > 0.0f)) return fail(TPT_ERR_INVALID_ARG, "point_tol must be > 0");
    tpt_scene* s = h->scene;
    if (deform) {
        // the only entry point that reads the scene's world buffers
        if (!s->built) return fail(TPT_ERR_INVALID_ARG, "scene not built: tpt_temporal_deform reads its world vertices");
        const tpt_status bs = finish_pending(s);
        if (bs != TPT_OK) return bs;
    }
    // the snapshot is the previous call's only if that call was tpt_temporal_deform
    const bool snap_valid = deform && h->snap_verts.p && h->snap_serial == h->serial;
    ++h->serial;
    DeviceGuard g(s->device);
    hipStream_t st = s->stream;
    const int W = h->width, H = h->height;
    const size_t npix = (size_t)W * (size_t)H;
    tpt::TemporalArgs a{};
    const CameraConsts cc = camera_consts(cam);
    set_camera(a, cc);
    a.inv_w = 1.0f / (float)W;
    a.inv_h = 1.0f / (float)H;
    a.has_prev = h->valid ? 1 : 0;
    std::memcpy(a.prev_inv, h->prev_inv, sizeof a.prev_inv);
    std::memcpy(a.prev_origin, h->prev.origin, sizeof a.prev_origin);
    a.prev_sensor_w = h->prev.sensor_w;
    a.prev_sensor_h = h->prev.sensor_h;
    a.prev_half_sw = h->prev.half_sw;
    a.prev_half_sh = h->prev.half_sh;
    a.width = W;
    a.height = H;
    a.demodulate = demod ? 1 : 0;
    a.tiles = (p->flags & TPT_TEMPORAL_TILES) ? 1 : 0;
    a.alpha = p->alpha;
    a.depth_tol = p->depth_tol;
    a.normal_min = p->normal_min;
    a.max_history = (float)p->max_history;
    // host buffers are staged on the device: inputs go up, outputs come back
    Staging sg(st);
    HIP_OR_FAIL(sg.in(h->st_rad, radiance_in, 3 * npix, &a.radiance_in));
    HIP_OR_FAIL(sg.in(h->st_f3[0], demod ? guides->albedo : nullptr, 3 * npix, &a.albedo));
    HIP_OR_FAIL(sg.in(h->st_f3[1], guides->normal, 3 * npix, &a.normal));
    HIP_OR_FAIL(sg.in(h->st_depth, guides->depth, npix, &a.depth));
    HIP_OR_FAIL(sg.in(h->st_mtl, guides->material, npix, &a.material));
    tpt::MotionArgs mo{};
    if (motion) {
        // every object's way back into the previous frame's world; without a previous frame the
        // kernel reads none of it
        const size_t nrec = (size_t)s->n_objects * tpt::kMotionRecordFloats;
        const float* now = s->h_vert_trans.data();
        (void)tpt_motion_matrices((uint32_t)s->n_objects, h->valid ? h->prev_vert_trans.data() : now, now,
                                  h->h_records.p);
        HIP_OR_FAIL(hipMemcpyAsync(h->records.p, h->h_records.p, nrec * sizeof(float), hipMemcpyHostToDevice, st));
        mo.records = reinterpret_cast<const float4*>(h->records.p);
        mo.face_object = h->face_object.p;
        mo.n_faces = s->n_faces;
        HIP_OR_FAIL(sg.in(h->st_face, guides->face, npix, &mo.face));
        HIP_OR_FAIL(sg.out(h->st_motion, motion_out, 2 * npix, &mo.motion_out));
    }
    tpt::DeformArgs de{};
    const size_t nv3 = 3 * (size_t)s->n_vertices;
    if (deform) {
        HIP_OR_FAIL(h->snap_verts.alloc(nv3));
        HIP_OR_FAIL(h->snap_norms.alloc(nv3));
        de.indices = s->indices.p;
        de.wverts = s->wverts.p;
        de.wnorms = s->wnorms.p;
        de.prev_wverts = h->snap_verts.p;
        de.prev_wnorms = h->snap_norms.p;
        de.n_faces = s->n_faces;
        de.snap_valid = snap_valid ? 1 : 0;
        HIP_OR_FAIL(sg.in(h->st_face, guides->face, npix, &de.face));
        HIP_OR_FAIL(sg.out(h->st_motion, motion_out, 2 * npix, &de.motion_out));
    }
    tpt::TemporalPathArgs pa{};
    if (path) {
        for (auto& plane : h->points)
            if (!plane.p) {   // the first call on this history: the fourth plane, zeroed once
                HIP_OR_FAIL(plane.alloc(npix));
                HIP_OR_FAIL(hipMemsetAsync(plane.p, 0, npix * sizeof(float4), st));
            }
        pa.point_tol = path->point_tol;
        HIP_OR_FAIL(sg.in(h->st_bounces, path->bounces, npix, &pa.bounces));
        HIP_OR_FAIL(sg.in(h->st_points, path->points, 3 * npix, &pa.points));
    }
    // radiance in and out share st_rad: a lane reads its pixel before it writes it
    HIP_OR_FAIL(sg.out(h->st_rad, radiance_out, 3 * npix, &a.radiance_out));
    HIP_OR_FAIL(sg.out(h->st_var, variance_out, npix, &a.variance_out));
    HIP_OR_FAIL(sg.out(h->st_len, history_len_out, npix, &a.history_out));
    // alpha is untouched: the caller's bytes go up first
    HIP_OR_FAIL(sg.inout(h->st_bgra, bgra_out, 4 * npix, &a.bgra));
    const int from = h->cur, to = h->cur ^ 1;
    for (int k = 0; k < 3; ++k) {
        a.prev[k] = h->state[from][k].p;
        a.next[k] = h->state[to][k].p;
    }
    pa.prev_points = h->points[from].p;
    pa.next_points = h->points[to].p;
    a.reprojected = h->count.set(0);
    HIP_OR_FAIL(h->count.zero(st));
    const bool clip = h->clip_on;
    tpt::ClipArgs cl{};
    if (clip) {
        // the box of this frame's colours, from the staged device copies of the inputs and ahead of
        // the temporal kernel: radiance_out may be radiance_in
        for (auto& plane : h->clip_planes) HIP_OR_FAIL(plane.alloc(npix));
        HIP_OR_FAIL(h->clip_count.alloc(2));
        tpt::ClipBoxArgs b{};
        b.width = W;
        b.height = H;
        b.radius = h->clip.radius;
        b.demodulate = a.demodulate;
        b.depth_tol = a.depth_tol;
        b.normal_min = a.normal_min;
        b.gamma = h->clip.gamma;
        b.radiance_in = a.radiance_in;
        b.albedo = a.albedo;
        b.normal = a.normal;
        b.depth = a.depth;
        b.material = a.material;
        b.bounces = path ? pa.bounces : nullptr;
        b.lo = h->clip_planes[0].p;
        b.hi = h->clip_planes[1].p;
        b.boxed = h->clip_count.set(0);
        cl.lo = b.lo;
        cl.hi = b.hi;
        cl.clip_history = (float)h->clip.max_history;
        cl.clipped = h->clip_count.set(1);
        HIP_OR_FAIL(h->clip_count.zero(st));
        HIP_OR_FAIL(hipEventRecord(h->clip_ev[0], st));
        HIP_OR_FAIL(tpt::launch_clip_box(b, st));
        HIP_OR_FAIL(hipEventRecord(h->clip_ev[1], st));
    }
    HIP_OR_FAIL(hipEventRecord(h->ev[0], st));
    HIP_OR_FAIL(tpt::launch_temporal(a, motion ? &mo : nullptr, path ? &pa : nullptr, deform ? &de : nullptr,
                                     clip ? &cl : nullptr, st));
    HIP_OR_FAIL(hipEventRecord(h->ev[1], st));
    if (deform) {   // the world buffers as this call saw them, for the next one
        HIP_OR_FAIL(hipMemcpyAsync(h->snap_verts.p, s->wverts.p, nv3 * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIP_OR_FAIL(hipMemcpyAsync(h->snap_norms.p, s->wnorms.p, nv3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    HIP_OR_FAIL(sg.finish());
    HIP_OR_FAIL(h->count.fetch(st));
    if (clip) HIP_OR_FAIL(h->clip_count.fetch(st));
    HIP_OR_FAIL(hipStreamSynchronize(st));
    // the new state, this camera and the scene's object transforms replace the old
    h->prev_vert_trans = s->h_vert_trans;
    h->cur = to;
    h->valid = true;
    if (!invert4(cam->c2w, h->prev_inv)) h->valid = false;   // a singular c2w: nothing can be reprojected into it
    h->prev = cc;
    if (deform) h->snap_serial = h->serial;
    h->clip_stats = tpt_clip_stats{};
    if (clip) {
        HIP_OR_FAIL(elapsed_ms(h->clip_ev[0], h->clip_ev[1], &h->clip_stats.box_ms));
        h->clip_stats.boxed = h->clip_count.sum(0);
        h->clip_stats.clipped = h->clip_count.sum(1);
    }
    if (stats) {
        HIP_OR_FAIL(elapsed_ms(h->ev[0], h->ev[1], &stats->kernel_ms));
        stats->reprojected = h->count.sum(0);
    }
    return TPT_OK;
}

tpt_status tpt_temporal(tpt_history* h, const tpt_camera* cam, const float* radiance_in, const tpt_aov* guides,
                        const tpt_temporal_params* p, float* radiance_out, float* variance_out,
                        float* history_len_out, uint8_t* bgra_out, tpt_temporal_stats* stats) {
    return temporal_pass(h, cam, radiance_in, guides, p, radiance_out, variance_out, history_len_out, nullptr, bgra_out,
                         stats, TemporalKind::Plain);
}

tpt_status tpt_temporal_motion(tpt_history* h, const tpt_camera* cam, const float* radiance_in, const tpt_aov* guides,
                               const tpt_temporal_params* p, float* radiance_out, float* variance_out,
                               float* history_len_out, float* motion_out, uint8_t* bgra_out,
                               tpt_temporal_stats* stats) {
    return temporal_pass(h, cam, radiance_in, guides, p, radiance_out, variance_out, history_len_out, motion_out,
                         bgra_out, stats, TemporalKind::Motion);
}

// tpt_temporal for a scene whose vertices moved (post.hip k_temporal with DeformArgs; DESIGN.md
// section 5 "Deforming meshes").
tpt_status tpt_temporal_deform(tpt_history* h, const tpt_camera* cam, const float* radiance_in, const tpt_aov* guides,
                               const tpt_temporal_params* p, float* radiance_out, float* variance_out,
                               float* history_len_out, float* motion_out, uint8_t* bgra_out,
                               tpt_temporal_stats* stats) {
    return temporal_pass(h, cam, radiance_in, guides, p, radiance_out, variance_out, history_len_out, motion_out,
                         bgra_out, stats, TemporalKind::Deform);
}

// tpt_temporal on mirror-path guides (post.hip k_temporal with TemporalPathArgs; DESIGN.md
// section 5 "Temporal accumulation through mirrors").
tpt_status tpt_temporal_path(tpt_history* h, const tpt_camera* cam, const float* radiance_in, const tpt_aov* path_guides,
                             const int32_t* bounces, const float* points, const tpt_temporal_path_params* p,
                             float* radiance_out, float* variance_out, float* history_len_out, uint8_t* bgra_out,
                             tpt_temporal_stats* stats) {
    if (!p) return fail(TPT_ERR_INVALID_ARG, "null params");
    const tpt_temporal_params tp{p->alpha, p->depth_tol, p->normal_min, p->max_history, p->flags};
    const PathInputs path{bounces, points, p->point_tol};
    return temporal_pass(h, cam, radiance_in, path_guides, &tp, radiance_out, variance_out, history_len_out, nullptr,
                         bgra_out, stats, TemporalKind::Path, &path);
}

// The variance-guided a-trous filter (post.hip k_svgf_*; DESIGN.md section 5
// "Post-pass"): pack into plane 0, the spatial variance estimate into plane 1, one
// launch per iteration between the two, resolve.  Where no pixel can be short (a
// variance without history lengths) the estimate is not launched.
tpt_status tpt_denoise_svgf(tpt_scene* s, int32_t W, int32_t H, const float* radiance_in, const tpt_aov* guides,
                            const float* variance_in, const float* history_len_in, const tpt_svgf_params* p,
                            float* radiance_out, float* variance_out, uint8_t* bgra_out, tpt_svgf_stats* stats) {
    if (!s) return fail(TPT_ERR_INVALID_ARG, "null scene");
    if (!radiance_in) return fail(TPT_ERR_INVALID_ARG, "null radiance_in");
    if (!guides) return fail(TPT_ERR_INVALID_ARG, "null guides");
    if (!p) return fail(TPT_ERR_INVALID_ARG, "null params");
    if (p->flags & ~(TPT_SVGF_DEMODULATE | TPT_SVGF_DIRECT)) return fail(TPT_ERR_INVALID_ARG, "unknown svgf flags");
    const bool demod = (p->flags & TPT_SVGF_DEMODULATE) != 0;
    if (!guides->normal || !guides->depth)
        return fail(TPT_ERR_INVALID_ARG, "the variance-guided filter needs the normal and depth guides");
    if (demod && !guides->albedo) return fail(TPT_ERR_INVALID_ARG, "TPT_SVGF_DEMODULATE needs the albedo guides");
    if (history_len_in && !variance_in)
        return fail(TPT_ERR_INVALID_ARG, "history_len_in needs a variance_in");
    if (W <= 0 || H <= 0) return fail(TPT_ERR_INVALID_ARG, "bad frame size: width and height must be > 0");
    if (p->iterations < 0 || p->iterations > 8) return fail(TPT_ERR_INVALID_ARG, "iterations must be 0..8");
    if (!(p->sigma_lum > 0.0f) || !(p->sigma_normal > 0.0f) || !(p->sigma_depth > 0.0f))
        return fail(TPT_ERR_INVALID_ARG, "sigma_lum, sigma_normal and sigma_depth must be > 0");
    if (p->min_history < 1 || p->min_history > 65536) return fail(TPT_ERR_INVALID_ARG, "min_history must be 1..65536");
    if (!radiance_out && !bgra_out) return fail(TPT_ERR_INVALID_ARG, "no output buffer: radiance_out and bgra_out are null");
    DeviceGuard g(s->device);
    hipStream_t st = s->stream;
    const size_t npix = (size_t)W * (size_t)H;
    HIP_OR_FAIL(s->dn_color[0].alloc(npix));
    HIP_OR_FAIL(s->dn_color[1].alloc(npix));
    HIP_OR_FAIL(s->dn_guide.alloc(npix));
    HIP_OR_FAIL(s->sv_count.alloc(1));
    const FilterConsts fc = filter_consts(p->sigma_normal, p->sigma_depth, p->flags & TPT_SVGF_DIRECT);
    tpt::SvgfArgs d{};
    d.npix = npix;
    d.width = W;
    d.height = H;
    d.demodulate = demod ? 1 : 0;
    d.passthrough = p->iterations == 0 ? 1 : 0;   // the input bit for bit, so no demodulation round trip
    d.min_history = (float)p->min_history;
    d.inv_sn2 = fc.inv_sn2;
    d.sz2 = fc.sz2;
    d.guide = s->dn_guide.p;
    d.estimated = s->sv_count.set(0);
    Staging sg(st);
    HIP_OR_FAIL(sg.in(s->dn_rad, radiance_in, 3 * npix, &d.radiance_in));
    HIP_OR_FAIL(sg.in(s->dn_f3[0], demod ? guides->albedo : nullptr, 3 * npix, &d.albedo));
    HIP_OR_FAIL(sg.in(s->dn_f3[1], guides->normal, 3 * npix, &d.normal));
    HIP_OR_FAIL(sg.in(s->dn_depth, guides->depth, npix, &d.depth));
    HIP_OR_FAIL(sg.in(s->sv_var, variance_in, npix, &d.variance_in));
    HIP_OR_FAIL(sg.in(s->sv_len, history_len_in, npix, &d.history_len));
    // radiance in and out share dn_rad, variance in and out sv_var: pack has read them by
    // the time resolve writes them (iterations 0: resolve's lane reads its pixel, then writes it)
    HIP_OR_FAIL(sg.out(s->dn_rad, radiance_out, 3 * npix, &d.radiance_out));
    HIP_OR_FAIL(sg.out(s->sv_var, variance_out, npix, &d.variance_out));
    // alpha is untouched: the caller's bytes go up first
    HIP_OR_FAIL(sg.inout(s->dn_bgra, bgra_out, 4 * npix, &d.bgra));
    HIP_OR_FAIL(s->sv_count.zero(st));
    HIP_OR_FAIL(hipEventRecord(s->ev[0], st));
    d.dst = s->dn_color[0].p;
    HIP_OR_FAIL(tpt::launch_svgf_pack(d, st));
    HIP_OR_FAIL(hipEventRecord(s->ev[1], st));
    int cur = 0;   // the plane that holds (c_i, v_i)
    if (!(variance_in && !history_len_in)) {
        d.src = s->dn_color[0].p;
        d.dst = s->dn_color[1].p;
        HIP_OR_FAIL(tpt::launch_svgf_estimate(d, st));
        cur = 1;
    }
    HIP_OR_FAIL(hipEventRecord(s->ev[2], st));
    tpt::SvgfFilterArgs f{};
    f.guide = s->dn_guide.p;
    f.width = W;
    f.height = H;
    f.sigma_lum = p->sigma_lum;
    f.inv_sn2 = fc.inv_sn2;
    f.sz2 = fc.sz2;
    for (int i = 0; i < p->iterations; ++i) {
        f.src = s->dn_color[cur].p;
        f.dst = s->dn_color[cur ^ 1].p;
        f.step = 1 << i;
        HIP_OR_FAIL(tpt::launch_svgf_filter(f, fc.use_lds, st));
        cur ^= 1;
    }
    HIP_OR_FAIL(hipEventRecord(s->ev[3], st));
    d.src = s->dn_color[cur].p;
    HIP_OR_FAIL(tpt::launch_svgf_resolve(d, st));
    HIP_OR_FAIL(hipEventRecord(s->ev[4], st));
    HIP_OR_FAIL(sg.finish());
    HIP_OR_FAIL(s->sv_count.fetch(st));
    HIP_OR_FAIL(hipStreamSynchronize(st));
    if (stats) {
        HIP_OR_FAIL(elapsed_ms(s->ev[0], s->ev[1], &stats->pack_ms));
        HIP_OR_FAIL(elapsed_ms(s->ev[1], s->ev[2], &stats->estimate_ms));
        HIP_OR_FAIL(elapsed_ms(s->ev[2], s->ev[3], &stats->filter_ms));
        HIP_OR_FAIL(elapsed_ms(s->ev[3], s->ev[4], &stats->resolve_ms));
        stats->estimated = s->sv_count.sum(0);
    }
    return TPT_OK;
}

// Guided upsampling (post.hip k_upsample; DESIGN.md section 5 "Guided upsampling"): one launch,
// no scratch plane.  Host buffers are staged in the scene's buffers: the full-size guides and the
// outputs in tpt_denoise's (the material in aov_i[1]), the low-size guides in tpt_render_aov's,
// the low-size radiance in up_rad.
tpt_status tpt_upsample(tpt_scene* s, int32_t wl, int32_t hl, const float* radiance_low, const tpt_aov* guides_low,
                        int32_t W, int32_t H, const tpt_aov* guides, const tpt_upsample_params* p,
                        float* radiance_out, uint8_t* bgra_out, tpt_upsample_stats* stats) {
    if (!s) return fail(TPT_ERR_INVALID_ARG, "null scene");
    if (!radiance_low) return fail(TPT_ERR_INVALID_ARG, "null radiance_low");
    if (!guides_low || !guides) return fail(TPT_ERR_INVALID_ARG, "null guides");
    if (!p) return fail(TPT_ERR_INVALID_ARG, "null params");
    if (p->flags & ~TPT_UPSAMPLE_DEMODULATE) return fail(TPT_ERR_INVALID_ARG, "unknown upsample flags");
    const bool demod = (p->flags & TPT_UPSAMPLE_DEMODULATE) != 0;
    for (const tpt_aov* g : {guides_low, guides}) {
        if (!g->normal || !g->depth || !g->material)
            return fail(TPT_ERR_INVALID_ARG, "upsampling needs the normal, depth and material guides at both sizes");
        if (demod && !g->albedo)
            return fail(TPT_ERR_INVALID_ARG, "TPT_UPSAMPLE_DEMODULATE needs the albedo guides at both sizes");
    }
    constexpr int32_t kMaxSide = 1048576;   // tpt_render_adaptive's
    if (wl <= 0 || hl <= 0 || W <= 0 || H <= 0) return fail(TPT_ERR_INVALID_ARG, "bad frame size: every side must be > 0");
    if (W > kMaxSide || H > kMaxSide) return fail(TPT_ERR_INVALID_ARG, "bad frame size: a side above 1048576");
    if (wl > W || hl > H) return fail(TPT_ERR_INVALID_ARG, "the low size is larger than the full size");
    if (!(p->sigma_normal > 0.0f) || !(p->sigma_depth > 0.0f))
        return fail(TPT_ERR_INVALID_ARG, "sigma_normal and sigma_depth must be > 0");
    if (!radiance_out && !bgra_out) return fail(TPT_ERR_INVALID_ARG, "no output buffer: radiance_out and bgra_out are null");
    DeviceGuard g(s->device);
    hipStream_t st = s->stream;
    const size_t npl = (size_t)wl * (size_t)hl, npix = (size_t)W * (size_t)H;
    HIP_OR_FAIL(s->up_count.alloc(1));
    const FilterConsts fc = filter_consts(p->sigma_normal, p->sigma_depth, false);
    tpt::UpsampleArgs a{};
    a.low_width = wl;
    a.low_height = hl;
    a.width = W;
    a.height = H;
    a.demodulate = demod ? 1 : 0;
    a.inv_sn2 = fc.inv_sn2;
    a.sz2 = fc.sz2;
    a.fallback = s->up_count.set(0);
    Staging sg(st);
    HIP_OR_FAIL(sg.in(s->up_rad, radiance_low, 3 * npl, &a.radiance_low));
    HIP_OR_FAIL(sg.in(s->aov_f3[0], demod ? guides_low->albedo : nullptr, 3 * npl, &a.albedo_low));
    HIP_OR_FAIL(sg.in(s->aov_f3[1], guides_low->normal, 3 * npl, &a.normal_low));
    HIP_OR_FAIL(sg.in(s->aov_depth, guides_low->depth, npl, &a.depth_low));
    HIP_OR_FAIL(sg.in(s->aov_i[0], guides_low->material, npl, &a.material_low));
    HIP_OR_FAIL(sg.in(s->dn_f3[0], demod ? guides->albedo : nullptr, 3 * npix, &a.albedo));
    HIP_OR_FAIL(sg.in(s->dn_f3[1], guides->normal, 3 * npix, &a.normal));
    HIP_OR_FAIL(sg.in(s->dn_depth, guides->depth, npix, &a.depth));
    HIP_OR_FAIL(sg.in(s->aov_i[1], guides->material, npix, &a.material));
    HIP_OR_FAIL(sg.out(s->dn_rad, radiance_out, 3 * npix, &a.radiance_out));
    // alpha is untouched: the caller's bytes go up first
    HIP_OR_FAIL(sg.inout(s->dn_bgra, bgra_out, 4 * npix, &a.bgra));
    HIP_OR_FAIL(s->up_count.zero(st));
    HIP_OR_FAIL(hipEventRecord(s->ev[0], st));
    HIP_OR_FAIL(tpt::launch_upsample(a, st));
    HIP_OR_FAIL(hipEventRecord(s->ev[1], st));
    HIP_OR_FAIL(sg.finish());
    HIP_OR_FAIL(s->up_count.fetch(st));
    HIP_OR_FAIL(hipStreamSynchronize(st));
    if (stats) {
        HIP_OR_FAIL(elapsed_ms(s->ev[0], s->ev[1], &stats->kernel_ms));
        stats->fallback = s->up_count.sum(0);
    }
    return TPT_OK;
}

// Tone mapping (tonemap.hip; DESIGN.md section 5 "Tone mapping").  The exposure handle keeps one
// ExposureBlock on the device; whether its `s` is a state is known here.
tpt_status tpt_exposure_create(tpt_scene* s, tpt_exposure** out) {
    if (!s) return fail(TPT_ERR_INVALID_ARG, "null scene");
    if (!out) return fail(TPT_ERR_INVALID_ARG, "null out");
    DeviceGuard g(s->device);
    std::unique_ptr<tpt_exposure> x(new tpt_exposure);
    x->scene = s;
    x->device = s->device;
    HIP_OR_FAIL(x->block.alloc(1));
    HIP_OR_FAIL(hipMemsetAsync(x->block.p, 0, sizeof(tpt::ExposureBlock), s->stream));
    HIP_OR_FAIL(hipStreamSynchronize(s->stream));
    *out = x.release();
    return TPT_OK;
}

tpt_status tpt_exposure_reset(tpt_exposure* x) {
    if (!x) return fail(TPT_ERR_INVALID_ARG, "null exposure");
    x->valid = false;
    return TPT_OK;
}

void tpt_exposure_destroy(tpt_exposure* x) {
    if (!x) return;
    DeviceGuard g(x->device);
    delete x;
}

tpt_status tpt_exposure_histogram(const tpt_exposure* x, uint64_t* bins256) {
    if (!x) return fail(TPT_ERR_INVALID_ARG, "null exposure");
    if (!bins256) return fail(TPT_ERR_INVALID_ARG, "null bins256");
    DeviceGuard g(x->device);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the bins are copied as they are");
    HIP_OR_FAIL(hipMemcpyAsync(bins256, x->block.p->hist, 256 * sizeof(uint64_t), hipMemcpyDeviceToHost, x->scene->stream));
    HIP_OR_FAIL(hipStreamSynchronize(x->scene->stream));
    return TPT_OK;
}

tpt_status tpt_exposure_measure_ms(const tpt_exposure* x, double* ms) {
    if (!x) return fail(TPT_ERR_INVALID_ARG, "null exposure");
    if (!ms) return fail(TPT_ERR_INVALID_ARG, "null ms");
    *ms = x->measure_ms;
    return TPT_OK;
}

// Under AUTO: histogram, measurement, map; the scale stays on the device between them and comes
// back with the figures once the map kernel is enqueued.  Otherwise the map kernel alone.
tpt_status tpt_tonemap(tpt_scene* s, tpt_exposure* x, int32_t W, int32_t H, const float* radiance_in,
                       const tpt_tonemap_params* p, float* radiance_out, uint8_t* bgra_out, tpt_tonemap_stats* stats) {
    if (!s) return fail(TPT_ERR_INVALID_ARG, "null scene");
    if (!radiance_in) return fail(TPT_ERR_INVALID_ARG, "null radiance_in");
    if (!p) return fail(TPT_ERR_INVALID_ARG, "null params");
    if (!radiance_out && !bgra_out) return fail(TPT_ERR_INVALID_ARG, "no output buffer: radiance_out and bgra_out are null");
    if (x && x->scene != s) return fail(TPT_ERR_INVALID_ARG, "the exposure belongs to another scene");
    constexpr int32_t kMaxSide = 1048576;   // tpt_upsample's
    if (W <= 0 || H <= 0) return fail(TPT_ERR_INVALID_ARG, "bad frame size: width and height must be > 0");
    if (W > kMaxSide || H > kMaxSide) return fail(TPT_ERR_INVALID_ARG, "bad frame size: a side above 1048576");
    const size_t npix = (size_t)W * (size_t)H;
    if (npix > ((size_t)1 << 31)) return fail(TPT_ERR_INVALID_ARG, "bad frame size: more than 2^31 pixels");
    if (p->op < TPT_TONEMAP_LINEAR || p->op > TPT_TONEMAP_ACES) return fail(TPT_ERR_INVALID_ARG, "unknown tone map op");
    if (p->transfer < TPT_TRANSFER_NONE || p->transfer > TPT_TRANSFER_GAMMA)
        return fail(TPT_ERR_INVALID_ARG, "unknown transfer function");
    if (p->flags & ~(TPT_TONEMAP_AUTO | TPT_TONEMAP_DITHER)) return fail(TPT_ERR_INVALID_ARG, "unknown tonemap flags");
    // (every comparison is false for a NaN)
    if (!std::isfinite(p->ev)) return fail(TPT_ERR_INVALID_ARG, "ev must be finite");
    if (!(p->white > 0.0f && std::isfinite(p->white))) return fail(TPT_ERR_INVALID_ARG, "white must be finite and > 0");
    if (!(p->gamma > 0.0f && std::isfinite(p->gamma))) return fail(TPT_ERR_INVALID_ARG, "gamma must be finite and > 0");
    if (!(p->key > 0.0f && std::isfinite(p->key))) return fail(TPT_ERR_INVALID_ARG, "key must be finite and > 0");
    if (!(p->p_low >= 0.0f && p->p_low < p->p_high && p->p_high <= 1.0f))
        return fail(TPT_ERR_INVALID_ARG, "p_low and p_high must be 0 <= p_low < p_high <= 1");
    if (!(p->min_ev <= p->max_ev && std::isfinite(p->min_ev) && std::isfinite(p->max_ev)))
        return fail(TPT_ERR_INVALID_ARG, "min_ev and max_ev must be finite, min_ev <= max_ev");
    if (!(p->rate > 0.0f && p->rate <= 1.0f)) return fail(TPT_ERR_INVALID_ARG, "rate must be in (0, 1]");
    const bool autoexp = (p->flags & TPT_TONEMAP_AUTO) != 0;
    DeviceGuard g(s->device);
    hipStream_t st = s->stream;
    tpt::TonemapArgs a{};
    a.width = W;
    a.height = H;
    a.op = p->op;
    a.transfer = p->transfer;
    a.dither = (p->flags & TPT_TONEMAP_DITHER) ? 1 : 0;
    a.white2 = p->white * p->white;
    a.inv_gamma = 1.0f / p->gamma;
    a.scale = std::exp2(p->ev);
    tpt::ExposureBlock* block = nullptr;
    if (autoexp) {
        HIP_OR_FAIL(s->tm_partials.alloc((size_t)tpt::kHistMaxBlocks * (tpt::kHistRowWords + 1)));
        HIP_OR_FAIL(s->tm_fetch.alloc(1));
        if (!x) HIP_OR_FAIL(s->tm_block.alloc(1));
        block = x ? x->block.p : s->tm_block.p;
    }
    Staging sg(st);
    HIP_OR_FAIL(sg.in(s->dn_rad, radiance_in, 3 * npix, &a.radiance_in));
    // radiance in and out share dn_rad: the histogram has read it, and a lane of the map kernel
    // reads its pixel before it writes it
    HIP_OR_FAIL(sg.out(s->dn_rad, radiance_out, 3 * npix, &a.radiance_out));
    // alpha is untouched: the caller's bytes go up first
    HIP_OR_FAIL(sg.inout(s->dn_bgra, bgra_out, 4 * npix, &a.bgra));
    if (autoexp) {
        tpt::HistArgs h{};
        h.radiance = a.radiance_in;
        h.npix = npix;
        h.partials = s->tm_partials.p;
        h.blocks = tpt::hist_blocks(npix);
        tpt::MeasureArgs m{};
        m.partials = h.partials;
        m.blocks = h.blocks;
        m.npix = npix;
        m.block = block;
        m.has_state = x && x->valid ? 1 : 0;
        m.p_low = p->p_low;
        m.p_high = p->p_high;
        m.key = p->key;
        m.min_ev = p->min_ev;
        m.max_ev = p->max_ev;
        m.rate = p->rate;
        m.ev = p->ev;
        a.block = block;
        HIP_OR_FAIL(hipEventRecord(s->ev[0], st));
        HIP_OR_FAIL(tpt::launch_histogram(h, st));
        HIP_OR_FAIL(hipEventRecord(s->ev[1], st));
        HIP_OR_FAIL(tpt::launch_measure(m, st));
    }
    HIP_OR_FAIL(hipEventRecord(s->ev[2], st));
    HIP_OR_FAIL(tpt::launch_tonemap(a, st));
    HIP_OR_FAIL(hipEventRecord(s->ev[3], st));
    if (autoexp)   // the figures: the block without its histogram
        HIP_OR_FAIL(hipMemcpyAsync(s->tm_fetch.p, block, offsetof(tpt::ExposureBlock, hist), hipMemcpyDeviceToHost, st));
    HIP_OR_FAIL(sg.finish());
    HIP_OR_FAIL(hipStreamSynchronize(st));
    tpt_tonemap_stats r{};
    r.log2_scale = p->ev;
    r.scale = a.scale;
    if (autoexp) {
        const tpt::ExposureBlock& f = *s->tm_fetch.p;
        r.log2_scale = f.log2_scale;
        r.scale = f.scale;
        r.log2_avg = f.log2_avg;
        r.counted = f.counted;
        r.dark = f.dark;
        r.nonfinite = f.nonfinite;
        HIP_OR_FAIL(elapsed_ms(s->ev[0], s->ev[1], &r.hist_ms));
        if (x) {
            if (f.counted > 0) x->valid = true;   // a frame without a counted pixel keeps what there was
            HIP_OR_FAIL(elapsed_ms(s->ev[1], s->ev[2], &x->measure_ms));
        }
    }
    HIP_OR_FAIL(elapsed_ms(s->ev[2], s->ev[3], &r.map_ms));
    if (stats) *stats = r;
    return TPT_OK;
}

}  // extern "C"
