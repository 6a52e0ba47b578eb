// api.cpp -- the C-ABI (include/tpt.h) over the HIP kernels: version, errors,
// read-backs, the debug entry points and the loaders.  The scene and env
// handles are in api_scene.cpp, tpt_render* in api_render.cpp, tpt_render_adaptive in
// api_adaptive.cpp, the post-pass in api_post.cpp; api_internal.hpp holds what they share.
//
// No exceptions cross the ABI: every entry point returns tpt_status and records
// a thread-local message for tpt_last_error().
#include <cstdlib>
#include <new>

#include "../kernels/kat.hpp"
#include "api_internal.hpp"

static thread_local std::string g_last_error;

tpt_status tpt::host::fail(tpt_status st, const std::string& msg) {
    g_last_error = msg;
    return st;
}

extern "C" {

const char* tpt_version(void) { return "tpt-mi355x 0.1 (gfx950)"; }

const char* tpt_last_error(void) { return g_last_error.c_str(); }

int tpt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

tpt_status tpt_image_load(const char* path, uint8_t** rgba, int32_t* width, int32_t* height) {
    if (!path || !rgba || !width || !height) return fail(TPT_ERR_INVALID_ARG, "null argument");
    *rgba = nullptr;
    std::vector<uint8_t> px;
    int w = 0, h = 0;
    try {
        tpt::load_image(path, px, w, h);
    } catch (const tpt::io_error& e) {
        return fail(TPT_ERR_IO, e.what());
    } catch (const std::exception& e) {
        return fail(TPT_ERR_PARSE, e.what());
    }
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(px.size()));
    if (!buf) return fail(TPT_ERR_OOM, "host allocation failed");
    std::memcpy(buf, px.data(), px.size());
    *rgba = buf;
    *width = w;
    *height = h;
    return TPT_OK;
}

void tpt_image_free(uint8_t* rgba) { std::free(rgba); }

tpt_status tpt_scene_read_bvh(tpt_scene* s, void* nodes36, int64_t* keys) {
    if (!s || !s->built) return fail(TPT_ERR_INVALID_ARG, "scene not built");
    DeviceGuard g(s->device);
    const size_t n = (size_t)s->n_faces;
    if (nodes36) HIP_OR_FAIL(hipMemcpy(nodes36, s->nodes36.p, 36 * (2 * n - 1), hipMemcpyDeviceToHost));
    if (keys) HIP_OR_FAIL(hipMemcpy(keys, s->keys_sorted.p, 8 * n, hipMemcpyDeviceToHost));
    return TPT_OK;
}

tpt_status tpt_scene_read_world(tpt_scene* s, float* wv, float* wn) {
    if (!s || !s->built) return fail(TPT_ERR_INVALID_ARG, "scene not built");
    DeviceGuard g(s->device);
    const size_t nv = (size_t)s->n_vertices;
    if (wv) HIP_OR_FAIL(hipMemcpy(wv, s->wverts.p, 12 * nv, hipMemcpyDeviceToHost));
    if (wn) HIP_OR_FAIL(hipMemcpy(wn, s->wnorms.p, 12 * nv, hipMemcpyDeviceToHost));
    return TPT_OK;
}

tpt_status tpt_debug_rng_init(int device, uint64_t seed, uint64_t first, uint32_t n, uint32_t* states) {
    if (!states && n) return fail(TPT_ERR_INVALID_ARG, "null output");
    int ndev = tpt_device_count();
    if (ndev <= 0) return fail(TPT_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(TPT_ERR_INVALID_ARG, "bad device index");
    DeviceGuard g(device);
    DevBuf<uint32_t> jumps, out;
    const auto& hj = host_jumps();
    HIP_OR_FAIL(jumps.upload(hj.data(), hj.size(), nullptr));
    HIP_OR_FAIL(out.alloc(6 * (size_t)std::max(n, 1u)));
    HIP_OR_FAIL(tpt::launch_rng_init_linear(jumps.p, seed, first, n, out.p, nullptr));
    HIP_OR_FAIL(hipDeviceSynchronize());
    if (n) HIP_OR_FAIL(hipMemcpy(states, out.p, 24 * (size_t)n, hipMemcpyDeviceToHost));
    return TPT_OK;
}

tpt_status tpt_debug_trace_rays(tpt_scene* s, uint32_t n, const float* o, const float* d, const int32_t* origin_fid,
                                int32_t mode, int32_t* hit, float* t, float* uv) {
    if (!s || !s->built) return fail(TPT_ERR_INVALID_ARG, "scene not built");
    if (mode < 0 || mode > 3) return fail(TPT_ERR_INVALID_ARG, "unknown trace mode");
    {
        const tpt_status bs = finish_pending(s);
        if (bs != TPT_OK) return bs;
    }
    if (n && (!o || !d || !hit || !t || !uv)) return fail(TPT_ERR_INVALID_ARG, "null argument");
    DeviceGuard g(s->device);
    DevBuf<float> dorg, ddir, dt, duv;
    DevBuf<int32_t> dhit, dofid;
    HIP_OR_FAIL(dorg.upload(o, 3 * (size_t)n, s->stream));
    if (origin_fid) {
        for (uint32_t i = 0; i < n; ++i)
            if (origin_fid[i] >= s->n_faces) return fail(TPT_ERR_INVALID_ARG, "origin face out of range");
        HIP_OR_FAIL(dofid.upload(origin_fid, n, s->stream));
    }
    HIP_OR_FAIL(ddir.upload(d, 3 * (size_t)n, s->stream));
    HIP_OR_FAIL(dhit.alloc(n));
    HIP_OR_FAIL(dt.alloc(n));
    HIP_OR_FAIL(duv.alloc(2 * (size_t)n));
    tpt::TraceArgs a{};
    fill_trace_args(s, nullptr, nullptr, a);
    HIP_OR_FAIL(tpt::launch_trace_rays(a, n, dorg.p, ddir.p, origin_fid ? dofid.p : nullptr, mode, dhit.p, dt.p, duv.p,
                                       s->stream));
    HIP_OR_FAIL(hipStreamSynchronize(s->stream));
    if (n) {
        HIP_OR_FAIL(hipMemcpy(hit, dhit.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
        HIP_OR_FAIL(hipMemcpy(t, dt.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
        HIP_OR_FAIL(hipMemcpy(uv, duv.p, 8 * (size_t)n, hipMemcpyDeviceToHost));
    }
    return TPT_OK;
}

tpt_status tpt_debug_step_latency(tpt_scene* s, uint32_t n, const float* o, const float* d, int32_t mode,
                                  int32_t flags, uint64_t* out) {
    if (!s || !s->built) return fail(TPT_ERR_INVALID_ARG, "scene not built");
    if (n > 64 || (n && (!o || !d || !out))) return fail(TPT_ERR_INVALID_ARG, "1..64 rays and outputs");
    if (mode < 0 || mode > 2)
        return fail(TPT_ERR_INVALID_ARG, "mode: 0 nodes in global memory, 1 in LDS, 2 four lanes per ray");
    if (mode == 2 && n > 16) return fail(TPT_ERR_INVALID_ARG, "four lanes per ray: at most 16 rays");
    {
        const tpt_status bs = finish_pending(s);
        if (bs != TPT_OK) return bs;
    }
    const int nodes_lds = mode == 1 ? s->n4 : (mode == 2 ? -1 : 0);
    if ((size_t)std::max(nodes_lds, 0) * 128 + 64 * 256 * sizeof(int) > 160 * 1024)
        return fail(TPT_ERR_INVALID_ARG, "the 4-wide tree does not fit in LDS");
    DeviceGuard g(s->device);
    DevBuf<float> dorg, ddir;
    DevBuf<unsigned long long> dout;
    HIP_OR_FAIL(dorg.upload(o, 3 * (size_t)std::max(n, 1u), s->stream));
    HIP_OR_FAIL(ddir.upload(d, 3 * (size_t)std::max(n, 1u), s->stream));
    HIP_OR_FAIL(dout.alloc(4 * 64));
    tpt::TraceArgs a{};
    fill_trace_args(s, nullptr, nullptr, a);
    if (mode == 2 && a.stack_depth + 3 > 64) return fail(TPT_ERR_INVALID_ARG, "four lanes per ray: stack too deep");
    if (flags & TPT_FLAG_FAST) {   // the tolerance-mode build, without the culling guards
        a.cull_eps = 0.0f;
        a.n_sliver_groups = 0;
        a.graze = 0;
        HIP_OR_FAIL(tpt_fast::launch_step_latency_ptr(&a, n, dorg.p, ddir.p, nodes_lds, dout.p, s->stream));
    } else {
        HIP_OR_FAIL(tpt::launch_step_latency_ptr(&a, n, dorg.p, ddir.p, nodes_lds, dout.p, s->stream));
    }
    HIP_OR_FAIL(hipStreamSynchronize(s->stream));
    HIP_OR_FAIL(hipMemcpy(out, dout.p, 4 * 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return TPT_OK;
}

int32_t tpt_debug_trace_wg_waves(int32_t family) { return tpt::trace_family_wgw(family); }

tpt_status tpt_debug_hot_kat(int device, int32_t op, uint32_t n, const float* in, float* out) {
    static const int kIn[4] = {12, 15, 16, 3}, kOut[4] = {2, 4, 6, 3};
    if (op < 0 || op > 3) return fail(TPT_ERR_INVALID_ARG, "unknown KAT op");
    if (n && (!in || !out)) return fail(TPT_ERR_INVALID_ARG, "null argument");
    int ndev = tpt_device_count();
    if (ndev <= 0) return fail(TPT_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(TPT_ERR_INVALID_ARG, "bad device index");
    DeviceGuard g(device);
    DevBuf<float> din, dout;
    HIP_OR_FAIL(din.upload(in, (size_t)kIn[op] * n, nullptr));
    HIP_OR_FAIL(dout.alloc((size_t)kOut[op] * std::max(n, 1u)));
    HIP_OR_FAIL(tpt::launch_hot_kat(op, n, din.p, dout.p, nullptr));
    HIP_OR_FAIL(hipDeviceSynchronize());
    if (n) HIP_OR_FAIL(hipMemcpy(out, dout.p, sizeof(float) * kOut[op] * (size_t)n, hipMemcpyDeviceToHost));
    return TPT_OK;
}

tpt_status tpt_debug_env_kat(int device, const tpt_env* env, int32_t op, uint32_t n, const float* in,
                             uint32_t* state, float* out) {
    if (op < 0 || op >= tpt::kEnvKatOps) return fail(TPT_ERR_INVALID_ARG, "unknown KAT op");
    if (n && (!in || !out)) return fail(TPT_ERR_INVALID_ARG, "null argument");
    if ((op == 3 || op == 4) && !env) return fail(TPT_ERR_INVALID_ARG, "this op needs an env");
    if (op == 4 && !(env->is_total > 0.0f)) return fail(TPT_ERR_INVALID_ARG, "the env's distribution is empty");
    if (op == 5 && n && !state) return fail(TPT_ERR_INVALID_ARG, "this op needs RNG states");
    if (op == 4)   // the searches index the tables by the uniforms: only (0, 1] (and 0) stays inside them
        for (uint32_t i = 0; i < n; ++i)
            for (int k = 3; k < 5; ++k)
                if (!(in[5 * (size_t)i + k] >= 0.0f && in[5 * (size_t)i + k] <= 1.0f))
                    return fail(TPT_ERR_INVALID_ARG, "x1 and x2 must lie in [0, 1]");
    int ndev = tpt_device_count();
    if (ndev <= 0) return fail(TPT_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(TPT_ERR_INVALID_ARG, "bad device index");
    if (env && env->device != device) return fail(TPT_ERR_INVALID_ARG, "the env lives on another device");
    DeviceGuard g(device);
    const size_t nin = (size_t)tpt::kEnvKatIn[op], nout = (size_t)tpt::kEnvKatOut[op];
    DevBuf<float> din, dout;
    DevBuf<uint32_t> dst;
    HIP_OR_FAIL(din.upload(in, nin * n, nullptr));
    HIP_OR_FAIL(dout.alloc(nout * std::max(n, 1u)));
    if (op == 5) HIP_OR_FAIL(dst.upload(state, 6 * (size_t)n, nullptr));
    tpt::TraceArgs a{};
    fill_env_args(env, a);
    HIP_OR_FAIL(tpt::launch_env_kat(a, op, n, din.p, dst.p, dout.p, nullptr));
    HIP_OR_FAIL(hipDeviceSynchronize());
    if (n) HIP_OR_FAIL(hipMemcpy(out, dout.p, sizeof(float) * nout * n, hipMemcpyDeviceToHost));
    if (n && op == 5) HIP_OR_FAIL(hipMemcpy(state, dst.p, sizeof(uint32_t) * 6 * (size_t)n, hipMemcpyDeviceToHost));
    return TPT_OK;
}

tpt_status tpt_gltf_load(const char* path, tpt_gltf** out) {
    if (!path || !out) return fail(TPT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    tpt_gltf* g = new (std::nothrow) tpt_gltf();
    if (!g) return fail(TPT_ERR_OOM, "host allocation failed");
    try {
        tpt::load_gltf(path, g->hs);
    } catch (const tpt::io_error& e) {
        delete g;
        return fail(TPT_ERR_IO, e.what());
    } catch (const std::exception& e) {
        delete g;
        return fail(TPT_ERR_PARSE, e.what());
    }
    *out = g;
    return TPT_OK;
}

tpt_status tpt_gltf_desc(const tpt_gltf* g, tpt_scene_desc* d, tpt_camera* cam) {
    if (!g || !d) return fail(TPT_ERR_INVALID_ARG, "null argument");
    const tpt::HostScene& h = g->hs;
    d->indices = h.indices.data();
    d->n_faces = (uint32_t)(h.indices.size() / 3);
    d->vertices = h.vertices.data();
    d->normals = h.normals.data();
    d->n_vertices = (uint32_t)(h.vertices.size() / 3);
    d->lut = h.lut.data();
    d->n_objects = (uint32_t)h.lut.size();
    d->vert_trans = h.vert_trans.data();
    d->normal_trans = h.normal_trans.data();
    d->materials = h.materials.empty() ? nullptr : h.materials.data();
    d->n_materials = (uint32_t)h.materials.size();
    d->lights = h.lights.empty() ? nullptr : h.lights.data();
    d->n_lights = (uint32_t)h.lights.size();
    d->flags = 0;
    if (cam) *cam = h.camera;
    return TPT_OK;
}

int tpt_gltf_missing_material(const tpt_gltf* g) { return g && g->hs.missing_material ? 1 : 0; }

void tpt_gltf_free(tpt_gltf* g) { delete g; }

}  // extern "C"
