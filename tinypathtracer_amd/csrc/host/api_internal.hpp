// api_internal.hpp -- what the translation units of the C-ABI share (api.cpp,
// api_scene.cpp, api_render.cpp, api_post.cpp): the error plumbing, the device
// and pinned-host buffers, the staging of caller buffers, the camera constants
// and the handle types behind include/tpt.h.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../common/device_api.hpp"
#include "../common/ptrig.hpp"
#include "../common/tpt_math.hpp"
#include "launch_plan.hpp"
#include "tpt.h"
#include "tpt_internal.hpp"

namespace tpt {
namespace host __attribute__((visibility("hidden"))) {

// No exceptions cross the ABI: every entry point returns tpt_status and records
// a thread-local message for tpt_last_error() (api.cpp).
tpt_status fail(tpt_status st, const std::string& msg);

#define HIP_OR_FAIL(expr)                                                                             \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(e_ == hipErrorOutOfMemory ? TPT_ERR_OOM : TPT_ERR_HIP,                         \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                          \
    } while (0)

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        if (count == n && p) return hipSuccess;
        release();
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    hipError_t upload(const T* src, size_t count, hipStream_t s) {
        hipError_t e = alloc(count);
        if (e != hipSuccess || count == 0) return e;
        return hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s);
    }
};

// Page-locked host memory (hipHostMalloc), grown on demand: the per-frame
// read-back of the leaf boxes runs at copy-engine speed instead of through a
// pageable bounce buffer.
template <class T>
struct HostPinned {
    T* p = nullptr;
    size_t n = 0;
    HostPinned() = default;
    HostPinned(const HostPinned&) = delete;
    HostPinned& operator=(const HostPinned&) = delete;
    ~HostPinned() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t alloc(size_t count) {
        if (count <= n && p) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipHostMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) n = count;
        return e;
    }
};

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev);
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
    }
};

// *owner (optional): the device that owns a device-memory pointer (-1 for host
// or managed memory, which every device can address).
inline bool is_device_ptr(const void* p, int* owner = nullptr) {
    if (owner) *owner = -1;
    if (!p) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const bool dev = attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
    if (attr.type == hipMemoryTypeDevice && owner) *owner = attr.device;
    return dev;
}

// A desc array in device memory (the reference's DeviceScene buffers) read back
// to the host, or the host array itself.  Returns the host view (null on a
// failed copy, with *err set).
template <typename T>
const T* host_view(const T* p, size_t n, std::vector<T>& tmp, hipError_t* err) {
    if (!p || n == 0 || !is_device_ptr(p)) return p;
    tmp.resize(n);
    const hipError_t e = hipMemcpy(tmp.data(), p, n * sizeof(T), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        *err = e;
        return nullptr;
    }
    return tmp.data();
}

// The staging rule of an entry point's caller buffers, written once: a device
// (or managed) pointer is used as it is; a host pointer gets the device buffer
// `buf` (kept by the scene / history between calls), the caller's bytes copied
// up before the kernels (in, inout) and the result copied back by finish() (out,
// inout).  A null pointer stays null.  *dev is what the kernel gets.  One pointer
// query per buffer; every copy on `st`, uploads in call order, finish()'s
// downloads in the order of the out / inout calls.  Two buffers of one size may
// share a `buf` where the kernels read the one before they write the other.
struct Staging {
    hipStream_t st;
    explicit Staging(hipStream_t s) : st(s) {}
    template <class T>
    hipError_t in(DevBuf<T>& buf, const T* p, size_t count, const T** dev) {
        return stage(buf, const_cast<T*>(p), count, true, false, const_cast<T**>(dev));
    }
    template <class T>
    hipError_t out(DevBuf<T>& buf, T* p, size_t count, T** dev) {
        return stage(buf, p, count, false, true, dev);
    }
    template <class T>
    hipError_t inout(DevBuf<T>& buf, T* p, size_t count, T** dev) {
        return stage(buf, p, count, true, true, dev);
    }
    // the device-to-host copies of what out / inout staged since the last finish()
    hipError_t finish() {
        hipError_t e = hipSuccess;
        for (int i = 0; i < n_back && e == hipSuccess; ++i)
            e = hipMemcpyAsync(back[i].host, back[i].dev, back[i].bytes, hipMemcpyDeviceToHost, st);
        n_back = 0;
        return e;
    }

private:
    struct Back {
        void* host;
        const void* dev;
        size_t bytes;
    };
    static constexpr int kMaxBack = 8;   // (tpt_render_aov_path_points has seven outputs)
    Back back[kMaxBack];
    int n_back = 0;
    template <class T>
    hipError_t stage(DevBuf<T>& buf, T* p, size_t count, bool up, bool down, T** dev) {
        *dev = p;
        if (!p || is_device_ptr(p)) return hipSuccess;
        if (down && n_back == kMaxBack) return hipErrorInvalidValue;
        hipError_t e = buf.alloc(count);
        if (e == hipSuccess && up) e = hipMemcpyAsync(buf.p, p, count * sizeof(T), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        if (down) back[n_back++] = {p, buf.p, count * sizeof(T)};
        *dev = buf.p;
        return hipSuccess;
    }
};

// The counters of the post-pass's statistics (post.hip spread_slot): `sets` sets of
// kTemporalSlots words, kTemporalSlotStride apart, on the device, and their pinned copy on the
// host.  zero() before the kernel, fetch() after it, sum() / max() once the stream has run.
struct SpreadCounters {
    static constexpr size_t kWords = (size_t)tpt::kTemporalSlots * tpt::kTemporalSlotStride;
    DevBuf<unsigned long long> dev;
    HostPinned<unsigned long long> host;
    hipError_t alloc(int sets) {
        const hipError_t e = dev.alloc((size_t)sets * kWords);
        return e != hipSuccess ? e : host.alloc((size_t)sets * kWords);
    }
    unsigned long long* set(int k) const { return dev.p + (size_t)k * kWords; }
    hipError_t zero(hipStream_t st) { return hipMemsetAsync(dev.p, 0, dev.n * sizeof(unsigned long long), st); }
    hipError_t fetch(hipStream_t st) {
        return hipMemcpyAsync(host.p, dev.p, dev.n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    }
    unsigned long long word(int set, int k) const { return host.p[(size_t)set * kWords + (size_t)k * tpt::kTemporalSlotStride]; }
    unsigned long long sum(int set) const {
        unsigned long long r = 0;
        for (int k = 0; k < tpt::kTemporalSlots; ++k) r += word(set, k);
        return r;
    }
    unsigned long long max(int set) const {
        unsigned long long r = 0;
        for (int k = 0; k < tpt::kTemporalSlots; ++k) r = std::max(r, word(set, k));
        return r;
    }
};

// The camera as the kernels take it (TraceArgs and TemporalArgs hold these fields
// under these names): reprojection is exact only while tpt_render_aov's rays and
// tpt_temporal's are built from the same bits, so both come from here.
struct CameraConsts {
    float c2w[16];
    float origin[3];                     // c2w * (0,0,0,1)
    float sensor_w, sensor_h;            // aspect*2tan(vfov/2), 2tan(vfov/2)
    float half_sw, half_sh;              // 0.5*sensor_w, 0.5*sensor_h
};
inline CameraConsts camera_consts(const tpt_camera* cam) {
    CameraConsts c;
    std::memcpy(c.c2w, cam->c2w, sizeof c.c2w);
    float r[4];
    tpt::mat4_vec4(cam->c2w, 0.0f, 0.0f, 0.0f, 1.0f, r);   // sampleRays :57
    c.origin[0] = r[0];
    c.origin[1] = r[1];
    c.origin[2] = r[2];
    const float tan_half = tpt::ptan(cam->vfov * 0.5f);    // :50-52
    c.sensor_h = 2.0f * tan_half;
    c.sensor_w = cam->aspect * c.sensor_h;
    c.half_sw = 0.5f * c.sensor_w;
    c.half_sh = 0.5f * c.sensor_h;
    return c;
}
template <class Args>
void set_camera(Args& a, const CameraConsts& c) {
    std::memcpy(a.c2w, c.c2w, sizeof a.c2w);
    std::memcpy(a.origin, c.origin, sizeof a.origin);
    a.sensor_w = c.sensor_w;
    a.sensor_h = c.sensor_h;
    a.half_sw = c.half_sw;
    a.half_sh = c.half_sh;
}

// The host half of a scene build: the SAH traversal trees over the LBVH's leaf
// boxes (wide_bvh.cpp).  Pure host work -- no HIP call, no access to the scene
// but its read-back staging -- so tpt_scene_build_async runs it on a thread of
// its own while the caller goes on (tpt_render enqueues the RNG
// initialisation, then waits for it: finish_pending).  One per scene, kept
// between builds with its work arrays and output buffers (no per-frame
// allocation to fault in).
struct HostTrees {
    size_t n = 0;
    const float* lbox = nullptr;      // 6 per leaf position (not owned: the scene's staging)
    const uint32_t* lemit = nullptr;  // per leaf position
    tpt::WideParams prm;
    int32_t lbvh_n4 = 0;      // the LBVH even-depth view's node count (inner4 when no SAH tree)
    bool timing = false;
    // results
    tpt::HostFloats w4, e4;
    int n4 = -1, need = 0, ne4 = -1, eneed = 0;
    tpt_status st = TPT_OK;
    std::string msg;
    tpt::WideWorkspace ws;
    std::thread th;
    ~HostTrees() { join(); }
    void join() {
        if (th.joinable()) th.join();
    }
    void reset_results() {
        n4 = -1;
        need = 0;
        ne4 = -1;
        eneed = 0;
        st = TPT_OK;
        msg.clear();
        prm.ws = &ws;
    }
    bool main_ok() const { return n4 > 0 && (size_t)n4 <= n - 1 && need <= 150; }
    int32_t base() const { return main_ok() ? n4 : lbvh_n4; }   // the emitter tree's first id
    bool emit_ok() const { return ne4 > 0 && (size_t)(base() + ne4) <= n - 1 && eneed <= 150; }
};

// Joins an asynchronous build's host half and uploads its trees (a no-op
// without one).  Every entry point that reads the traversal trees calls it
// (api_scene.cpp).
tpt_status finish_pending(tpt_scene* s, double* wait_ms = nullptr);
// the scene, the env and (cam non-null) the camera constants of a launch (api_render.cpp)
void fill_trace_args(tpt_scene* s, const tpt_env* env, const tpt_camera* cam, tpt::TraceArgs& a);
// the env's part of them alone (nullable env: no map, an empty distribution)
void fill_env_args(const tpt_env* env, tpt::TraceArgs& a);

}  // namespace host
}  // namespace tpt

using namespace tpt::host;

struct tpt_env {
    int device = 0;
    int w = 0, h = 0;
    DevBuf<uint32_t> texels;
    // importance-sampling tables (A15, TPT_FLAG_ENV_IS) over blocks of B x B
    // texels: block-row prefix sums, block-row sums, marginal prefix over block
    // rows; total <= 0 disables
    DevBuf<float> is_cond, is_row, is_marg;
    float is_total = 0.0f;
    int32_t is_b = 1, is_bw = 0, is_bh = 0;   // block side, blocks per row, block rows
    DevBuf<int32_t> is_guide_r, is_guide_c;   // guide tables of the two CDF searches (trace.hip lower_bound_guided)
    int32_t is_kr = 1, is_kc = 1;
};

struct tpt_scene {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[5] = {};                  // tpt_render uses four, tpt_denoise_svgf's four kernels all five
    int32_t n_faces = 0, n_vertices = 0, n_objects = 0, n_materials = 0, n_lights = 0;
    bool built = false;
    int32_t stack_depth = 0;
    int32_t boxes_finite = 0;
    int32_t any_emitter = 1;                // some triangle's material has emissionFactor != 0
    int32_t unwind_prune = 0;               // every baseColor component passes tpt::prune_color_ok (TraceArgs unwind_prune)
    int32_t n4 = 0;
    int32_t wide_tree = 0;                  // 1: inner4 holds the SAH 4-wide tree (wide_bvh.cpp)
    int32_t emit_root = -1;                 // inner4 id of the emissive-triangle tree's root (-1: none)
    float emit_box[24] = {};                // boxes around the emitters' leaf boxes (TraceArgs emit_box)
    int32_t n_emit_box = 0;
    int32_t slivers = 0;                    // sliver triangles (trace.hip "Culling"), re-tested after traversal
    int32_t n_sliver_groups = 0;
    DevBuf<float4> sliver_groups, sliver_list;
    float cull_eps = 0.0f;                  // absolute position slack of the t-culls
    uint32_t tree_depth = 0;
    int32_t build_threads = -1;             // SAH tree build threads (tpt_scene_set_build_threads)
    DevBuf<uint8_t> sliver_flags;           // k_sliver_scan outputs
    DevBuf<unsigned long long> coord_max;
    HostPinned<float> h_lbox;               // read-back staging of a build (leaf boxes, emitter flags,
    HostPinned<uint32_t> h_lemit;           // sliver flags + coord_max); declared before `trees`, which
    HostPinned<uint8_t> h_sliver;           // reads them and is destroyed (joined) first
    std::unique_ptr<HostTrees> trees;       // the host half of the builds
    bool pending = false;                   // tpt_scene_build_async's host half runs / is not uploaded yet
    uint32_t pending_need = 0;              // its stack bound before the trees
    // tpt_scene_refit: whether the device holds a complete full build (set where a build
    // completes, cleared where one starts; tpt_scene_set_* leave it), the level ranges of the two
    // 4-wide trees as inner4 ids (lv[l] .. lv[l + 1]; empty: none, or not level-ordered), the
    // tree cost as the last full build left it (measured by the first refit after it) and the
    // cost kernels' buffers
    bool resident = false;
    int32_t n_emit4 = 0;                    // nodes of the emissive-triangle tree (from emit_root)
    std::vector<int32_t> lv_main, lv_emit;
    bool cost_built_valid = false;
    double cost_built = 0.0;
    DevBuf<double> cost_terms, cost_out;    // per main-tree node; (sum, root area) as built and as refitted
    HostPinned<double> h_cost;
    HostPinned<float> h_eroot;              // the emissive tree's root node, read back for emit_box
    HostPinned<uint32_t> h_nonfinite;
    // inputs
    DevBuf<uint32_t> indices;
    DevBuf<float> vertices, normals, vert_trans, normal_trans;
    DevBuf<int2> lut;
    DevBuf<float4> mtl;
    DevBuf<tpt::DevLight> lights;
    DevBuf<uint32_t> jumps;
    // host copies: every object's local-to-world matrix as the device holds it (tpt_scene_create,
    // tpt_scene_set_transforms) and the objects' first faces, for the histories' motion records
    std::vector<float> h_vert_trans;
    std::vector<int32_t> h_lut_begin;
    // world + BVH
    DevBuf<float> wverts, wnorms, leaf_box, node_box;
    DevBuf<unsigned long long> keys, keys_sorted, bfs_keys, bfs_keys_sorted;
    DevBuf<uint32_t> fids, fids_sorted, parent, flags, max_depth, bfs_ids, bfs_ids_sorted, bfs_newid, emit;
    DevBuf<int2> children;
    DevBuf<uint8_t> sort_tmp, nodes36;
    DevBuf<float4> inner, inner4, tri, shade;
    // frame state
    DevBuf<uint32_t> rng;
    DevBuf<int32_t> credit;                 // run-ahead (TraceArgs::credit): one plane per frame, zero between calls
    DevBuf<float> accum, radiance_tmp;
    DevBuf<uint8_t> bgra_tmp;
    DevBuf<unsigned long long> counters, debug;
    size_t frame_pixels = 0;
    // progressive accumulation (TPT_FLAG_ACCUMULATE): the frame the rng/accum state belongs to
    bool acc_valid = false;
    int acc_w = 0, acc_h = 0, acc_rows = 0, acc_count = 0, acc_index = 0;
    std::vector<int32_t> acc_list;          // the explicit deal it was rendered with (empty: interleaved)
    uint64_t acc_spp = 0;
    // explicit band deals (tpt_params.band_list): the call's list, then each band
    // set's share of it (host copy kept until the call's copies have run)
    DevBuf<int32_t> band_lists;
    std::vector<int32_t> band_lists_h;
    DevBuf<unsigned long long> band_cost;   // per global band: summed wave life (tpt_params.band_cost)
    std::vector<unsigned long long> band_cost_h;
    // the chip, from hipDeviceProp_t: compute units, and the lanes the one-lane
    // trace variant keeps resident (CUs x 4 SIMDs x its waves per SIMD x 64)
    int32_t n_cu = 0;
    uint64_t resident_lanes = 0;
    std::vector<uint64_t> acc_seeds;        // one per frame of the batch
    // overlapped launch pipeline: extra streams (set k >= 1 of a frame's rows)
    // and a pool of per-launch timing events
    std::vector<hipStream_t> pipe;
    std::vector<hipEvent_t> lev;
    hipEvent_t pipe_ev[2 * tpt::kMaxPipe] = {};
    // wavefront variant (TPT_FLAG_WAVEFRONT, wavefront.hip): slot state, path
    // records, the two ray queues, the hit records, the control words
    DevBuf<uint32_t> wf_state, wf_ctl;
    DevBuf<float> wf_rec;
    DevBuf<float4> wf_q0, wf_q1, wf_hit;
    HostPinned<uint32_t> wf_count;
    hipEvent_t wf_ev[2] = {nullptr, nullptr};
    // post-pass (post.hip).  tpt_render_aov: device staging of host outputs.  tpt_denoise: the two
    // colour planes and the guide plane (float4 per pixel each), device staging of host inputs /
    // outputs.  All kept between calls, as the wavefront buffers are.
    DevBuf<float> aov_f3[2], aov_depth;     // albedo, normal; depth
    DevBuf<int32_t> aov_i[2];               // face, material
    DevBuf<float4> dn_color[2], dn_guide;
    DevBuf<float> dn_rad, dn_f3[2], dn_depth;   // radiance in / out; albedo, normal; depth
    DevBuf<uint8_t> dn_bgra;
    // tpt_denoise_svgf: the planes and staging above, and of its own the staging of the variance
    // (in and out share it), of the history length and the counters of SvgfArgs::estimated
    DevBuf<float> sv_var, sv_len;
    SpreadCounters sv_count;
    // tpt_render_aov_path: tpt_render_aov's staging above, and of its own the staging of the bounce
    // counts and the counters of AovPathArgs::followed (set 0) and ::deepest (set 1)
    DevBuf<int32_t> ap_bounces;
    SpreadCounters ap_count;
    DevBuf<float> ap_points;                // tpt_render_aov_path_points: the staging of the terminal points
    // tpt_upsample: no plane of its own.  Host buffers are staged in tpt_denoise's buffers (the
    // full-size guides and outputs, the material in aov_i[1]) and tpt_render_aov's (the low-size
    // guides); of its own the staging of the low-size radiance and the counters of
    // UpsampleArgs::fallback
    DevBuf<float> up_rad;
    SpreadCounters up_count;
    // tpt_tonemap: no plane of its own.  Host buffers are staged in tpt_denoise's dn_rad (in and out
    // share it) and dn_bgra; of its own the histogram kernel's partials, the exposure block of a
    // call without a tpt_exposure and the pinned copy of a call's figures
    DevBuf<uint32_t> tm_partials;
    DevBuf<tpt::ExposureBlock> tm_block;
    HostPinned<tpt::ExposureBlock> tm_fetch;
    // tpt_render_adaptive (adaptive.hip): the sums' snapshot at half a tile's samples (3 planes, 12 B
    // per pixel), the active tiles' list, the tiles' error estimates and sample counts, with pinned
    // host copies.  Kept between calls.
    DevBuf<float> ad_snap, ad_err;
    DevBuf<uint32_t> ad_tiles;
    DevBuf<int32_t> ad_spp;
    HostPinned<float> ad_err_h;
    HostPinned<uint32_t> ad_tiles_h;
    HostPinned<int32_t> ad_spp_h;

    ~tpt_scene() {
        DeviceGuard g(device);
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : lev)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : pipe_ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : wf_ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& q : pipe)
            if (q) (void)hipStreamDestroy(q);
        if (stream) (void)hipStreamDestroy(stream);
    }

    // streams for the n band sets and the fork/join events.  Every set needs a
    // hardware queue of its own: two streams on one queue run their launches
    // one after another (a process has GPU_MAX_HW_QUEUES = 4; measured on the
    // box, one or two idle streams created earlier in the process -- a
    // communicator's -- made two sets share a queue: -25 %).  The runtime
    // keeps a queue pool per stream priority, so the sets' streams are created
    // at the greatest priority, where nothing else in the process competes.
    hipError_t ensure_pipe(int n) {
        hipError_t e = hipSuccess;
        int lo = 0, hi = 0;
        e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        while (e == hipSuccess && (int)pipe.size() < n) {
            hipStream_t q = nullptr;
            e = hipStreamCreateWithPriority(&q, hipStreamNonBlocking, hi);
            if (e == hipSuccess) pipe.push_back(q);
        }
        for (int i = 0; e == hipSuccess && i < 2 * tpt::kMaxPipe; ++i)
            if (!pipe_ev[i]) e = hipEventCreateWithFlags(&pipe_ev[i], hipEventDisableTiming);
        return e;
    }
    hipError_t ensure_launch_events(size_t n) {
        hipError_t e = hipSuccess;
        while (e == hipSuccess && lev.size() < n) {
            hipEvent_t x = nullptr;
            e = hipEventCreate(&x);
            if (e == hipSuccess) lev.push_back(x);
        }
        return e;
    }
};

// tpt_tonemap's exposure across frames (tonemap.hip k_tm_measure): the adapted log2 scale, the last
// measured histogram and the last call's figures, on the device.
struct tpt_exposure {
    tpt_scene* scene = nullptr;             // the device and the stream; outlives the exposure
    int device = 0;
    DevBuf<tpt::ExposureBlock> block;
    bool valid = false;                     // false after create / reset: block.s is not a state
    double measure_ms = 0.0;                // the last AUTO call's measurement kernel
};

// Which of the four temporal entry points a call is: tpt_temporal, tpt_temporal_motion,
// tpt_temporal_path, tpt_temporal_deform.
enum class TemporalKind { Plain, Motion, Path, Deform };

// The temporal entry points' state (post.hip k_temporal): two sets of three float4 planes that
// ping-pong, the previous call's camera and object transforms, device staging of host buffers.
struct tpt_history {
    tpt_scene* scene = nullptr;             // the stream; outlives the history's last tpt_temporal
    int device = 0;
    int32_t width = 0, height = 0;
    DevBuf<float4> state[2][3];
    int cur = 0;                            // the set the last call wrote
    bool valid = false;                     // false after create / reset: no state
    float prev_inv[16] = {};                // inverse of the previous c2w, column-major
    CameraConsts prev = {};                 // the previous call's camera
    DevBuf<float> st_rad, st_f3[2], st_depth, st_var, st_len;
    DevBuf<int32_t> st_mtl;
    DevBuf<uint8_t> st_bgra;
    SpreadCounters count;                   // the reprojected pixels (TemporalArgs::reprojected)
    // tpt_temporal_motion: the scene's vert_trans as they were at the previous call (empty: no
    // state), the face -> object table (built once from the lut), the objects' records
    // (tpt_motion_matrices) on both sides, device staging of the face guide and of motion_out
    std::vector<float> prev_vert_trans;
    DevBuf<int32_t> face_object;
    DevBuf<float> records;
    HostPinned<float> h_records;
    DevBuf<int32_t> st_face;
    DevBuf<float> st_motion;
    // tpt_temporal_path: a fourth state plane per set, the paths' terminal points (allocated and
    // zeroed at the first call: +32 B per pixel), device staging of the bounce counts and the points
    DevBuf<float4> points[2];
    DevBuf<int32_t> st_bounces;
    DevBuf<float> st_points;
    // tpt_temporal_deform: the scene's world vertices and normals as they were at the end of the
    // last tpt_temporal_deform call (24 B per vertex, allocated at the first one).  Every call on
    // the history and every reset advances `serial`; the snapshot is the previous call's only
    // while snap_serial is still the current serial.
    DevBuf<float> snap_verts, snap_norms;
    uint64_t serial = 0, snap_serial = ~0ull;
    // tpt_history_set_clip: the setting (it survives a reset), k_clip_box's two planes (allocated at
    // the first clipped call: +32 B per pixel), the counters of the boxed (set 0) and the clipped
    // (set 1) pixels, the last call's figures and the box kernel's events
    bool clip_on = false;
    tpt_clip_params clip = {};
    DevBuf<float4> clip_planes[2];
    SpreadCounters clip_count;
    tpt_clip_stats clip_stats = {};
    hipEvent_t clip_ev[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};

    ~tpt_history() {
        DeviceGuard g(device);
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : clip_ev)
            if (e) (void)hipEventDestroy(e);
    }
};

