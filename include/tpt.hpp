// tpt.hpp -- C++ host API over the C-ABI (tpt.h), mirroring the reference's
// PathTracer / Scene / BVH / Camera classes:
//   include/path_tracer.h:16-35   PathTracer(), PathTracer(envFile), render(meshFile)
//   include/mesh.cuh:98-115       Scene(file, "gltf"), copySceneToDevice(), m_camera
//   include/bvh.cuh:60-68         BVH(size), construct(...), m_nodes, m_keys
//   include/camera.h:9-65         getVFov / getAspRatio / getNearPlane
// Errors throw std::runtime_error, as the reference's CUDA_CHECK and loader do
// (include/intellisense_cuda.h:14-20, src/mesh.cu:76,94,303).  Header-only:
// link against libtpt.so.
#pragma once

#include <cstdint>
#include <cstring>
#include <ctime>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "tpt.h"

namespace tpt {

inline void check(tpt_status st) {
    if (st != TPT_OK) throw std::runtime_error(std::string("tpt: ") + tpt_last_error());
}

struct Camera {
    tpt_camera c{};
    float getVFov() const { return c.vfov; }
    float getAspRatio() const { return c.aspect; }
    float getNearPlane() const { return c.znear; }
};

// BVHNode (include/bvh.cuh:52-58): 36 bytes
struct BVHNode {
    uint32_t parent;
    int32_t a, b;       // internal: left/right child; leaf: fid, placeHolder
    float bmin[3], bmax[3];
};
static_assert(sizeof(BVHNode) == 36, "BVHNode layout");
static_assert(sizeof(tpt_aov_path_params) == 8 && sizeof(tpt_aov_path_stats) == 24, "tpt_aov_path_* layout");
static_assert(sizeof(tpt_clip_params) == 16 && sizeof(tpt_clip_stats) == 24, "tpt_clip_* layout");

class DeviceScene;

class Scene {
public:
    Scene(const std::string& filename, const std::string& type) {
        if (type != "gltf") throw std::runtime_error("Unsupported file format. Only support .gltf file.");
        tpt_gltf* g = nullptr;
        check(tpt_gltf_load(filename.c_str(), &g));
        gltf_.reset(g);
        check(tpt_gltf_desc(gltf_.get(), &desc_, &m_camera.c));
    }
    DeviceScene copySceneToDevice(int device = 0) const;
    const tpt_scene_desc& desc() const { return desc_; }
    bool missingMaterial() const { return tpt_gltf_missing_material(gltf_.get()) != 0; }

    Camera m_camera;

private:
    struct Free {
        void operator()(tpt_gltf* g) const { tpt_gltf_free(g); }
    };
    std::unique_ptr<tpt_gltf, Free> gltf_;
    tpt_scene_desc desc_{};
};

class DeviceScene {
public:
    DeviceScene(const tpt_scene_desc& d, int device) : n_faces_(d.n_faces), n_vertices_(d.n_vertices) {
        tpt_scene* s = nullptr;
        check(tpt_scene_create(&d, device, &s));
        scene_.reset(s);
    }
    // World transform + LBVH on the device (path_tracer.cu:536-542)
    DeviceScene& build() {
        check(tpt_scene_build(scene_.get()));
        built_ = true;
        return *this;
    }
    // New local-to-world matrices for objects first, first + 1, ... (tpt_scene_set_transforms:
    // 16 floats each, column-major; normal_trans null: the loader's inverse transpose).  The
    // scene is unbuilt afterwards: build() comes next.
    DeviceScene& setTransforms(uint32_t first, uint32_t n_objects, const float* vert_trans,
                               const float* normal_trans = nullptr) {
        check(tpt_scene_set_transforms(scene_.get(), first, n_objects, vert_trans, normal_trans));
        built_ = false;
        return *this;
    }
    // New object-space positions (xyz each) for vertices first, first + 1, ...
    // (tpt_scene_set_vertices; normals null: the stored ones stay; host or device memory).  The
    // scene is unbuilt afterwards: build() comes next.
    DeviceScene& setVertices(uint32_t first, uint32_t n_vertices, const float* vertices,
                             const float* normals = nullptr) {
        check(tpt_scene_set_vertices(scene_.get(), first, n_vertices, vertices, normals));
        built_ = false;
        return *this;
    }
    // In place of build() after setVertices / setTransforms (tpt_scene_refit): the last full
    // build's topology with every box recomputed on the device; a full build where it must be.
    // stats->cost / cost_built is the caller's signal for a rebuild.
    DeviceScene& refit(tpt_refit_stats* stats = nullptr) {
        check(tpt_scene_refit(scene_.get(), stats));
        built_ = true;
        return *this;
    }
    bool built() const { return built_; }
    tpt_scene* handle() const { return scene_.get(); }
    uint32_t nFaces() const { return n_faces_; }
    uint32_t nVertices() const { return n_vertices_; }

private:
    struct Free {
        void operator()(tpt_scene* s) const { tpt_scene_destroy(s); }
    };
    std::unique_ptr<tpt_scene, Free> scene_;
    uint32_t n_faces_, n_vertices_;
    bool built_ = false;
};

inline DeviceScene Scene::copySceneToDevice(int device) const { return DeviceScene(desc_, device); }

struct BVH {
    BVH() = default;
    explicit BVH(size_t size) : m_nodes(size ? 2 * size - 1 : 0), m_keys(size) {}
    // Builds on the device and reads back the reference node array.
    void construct(DeviceScene& scene) {
        if (!scene.built()) scene.build();
        m_nodes.resize(2 * (size_t)scene.nFaces() - 1);
        m_keys.resize(scene.nFaces());
        check(tpt_scene_read_bvh(scene.handle(), m_nodes.data(), m_keys.data()));
    }
    std::vector<BVHNode> m_nodes;
    std::vector<int64_t> m_keys;
};

class EnvLight {
public:
    EnvLight() = default;
    // rgba: width*height*4, row 0 = top (image order); stored bottom-up like
    // FreeImage (picture.h:41-43).
    EnvLight(const uint8_t* rgba_top_down, int width, int height, int device = 0) {
        std::vector<uint8_t> flipped((size_t)width * height * 4);
        for (int y = 0; y < height; ++y)
            std::memcpy(&flipped[(size_t)y * width * 4], rgba_top_down + (size_t)(height - 1 - y) * width * 4,
                        (size_t)width * 4);
        tpt_env* e = nullptr;
        check(tpt_env_create(flipped.data(), width, height, device, &e));
        env_.reset(e, Free());
    }
    // EnvLight(file) (env_light.cuh:8-18): JPEG or binary PPM decoded natively
    // as FreeImage would (tpt_env_load); throws std::runtime_error like Picture.
    explicit EnvLight(const std::string& file, int device = 0) {
        tpt_env* e = nullptr;
        check(tpt_env_load(file.c_str(), device, &e));
        env_.reset(e, Free());
    }
    const tpt_env* handle() const { return env_.get(); }

private:
    struct Free {
        void operator()(tpt_env* e) const { tpt_env_destroy(e); }
    };
    std::shared_ptr<tpt_env> env_;
    friend class PathTracer;
};

struct Frame {
    int width = 0, height = 0;
    std::vector<uint8_t> bgra;     // row 0 = top (copyToFB layout), B,G,R,A
    std::vector<float> radiance;   // row 0 = bottom, color / spp
    tpt_stats stats{};
};

// First-hit feature buffers (tpt_aov) in host memory, row 0 = bottom
struct AOV {
    int width = 0, height = 0;
    std::vector<float> albedo, normal;   // 3 per pixel
    std::vector<float> depth;
    std::vector<int32_t> face, material;
    tpt_aov view() { return tpt_aov{albedo.data(), normal.data(), depth.data(), face.data(), material.data()}; }
};

// The hosts' denoiser defaults (DESIGN.md section 5 "Post-pass")
inline tpt_denoise_params defaultDenoise(int iterations = 5) {
    tpt_denoise_params p{};
    p.iterations = iterations;
    p.sigma_color = 4.0f;
    p.sigma_normal = 0.3f;
    p.sigma_depth = 0.05f;
    p.flags = TPT_DENOISE_DEMODULATE;
    return p;
}

// The hosts' temporal-accumulation defaults (DESIGN.md section 5 "Post-pass")
inline tpt_temporal_params defaultTemporal() {
    tpt_temporal_params p{};
    p.alpha = 0.1f;
    p.depth_tol = 0.1f;
    p.normal_min = 0.9f;
    p.max_history = 32;
    p.flags = TPT_TEMPORAL_DEMODULATE;
    return p;
}

// The hosts' defaults of accumulation through mirrors: defaultTemporal's, and point_tol by the
// sweep of tools/temporal_path_quality.py (DESIGN.md section 5 "Temporal accumulation through mirrors")
inline tpt_temporal_path_params defaultTemporalPath() {
    const tpt_temporal_params t = defaultTemporal();
    tpt_temporal_path_params p{};
    p.alpha = t.alpha;
    p.depth_tol = t.depth_tol;
    p.normal_min = t.normal_min;
    p.max_history = t.max_history;
    p.flags = t.flags;
    p.point_tol = 8.0f;
    return p;
}

// The hosts' defaults of history clipping (History::setClip), by the sweep of tools/clip_quality.py
// (DESIGN.md section 5 "History clipping")
inline tpt_clip_params defaultClip() {
    tpt_clip_params p{};
    p.radius = 1;
    p.gamma = 1.0f;
    p.max_history = 4;
    p.flags = 0;
    return p;
}

// The hosts' defaults of the variance-guided filter (DESIGN.md section 5 "Post-pass":
// sigma_lum by the sweep there, not the paper's 4)
inline tpt_svgf_params defaultSVGF(int iterations = 5) {
    tpt_svgf_params p{};
    p.iterations = iterations;
    p.sigma_lum = 0.5f;
    p.sigma_normal = 0.3f;
    p.sigma_depth = 0.05f;
    p.min_history = 4;
    p.flags = TPT_SVGF_DEMODULATE;
    return p;
}

// The hosts' defaults of guided upsampling (PathTracer::upsample), chosen by the sweep of
// tools/upsample_quality.py (DESIGN.md section 5 "Guided upsampling"), which started from
// defaultDenoise's sigmas and kept sigma_normal
inline tpt_upsample_params defaultUpsample() {
    tpt_upsample_params p{};
    p.sigma_normal = 0.3f;
    p.sigma_depth = 0.2f;
    p.flags = 0;
    return p;
}

// The low frame size of an integer scale: ceil(width / scale) x ceil(height / scale)
struct Size {
    int width = 0, height = 0;
};
inline Size lowSize(int width, int height, int scale) {
    if (width <= 0 || height <= 0 || scale <= 0) throw std::runtime_error("lowSize: width, height and scale must be > 0");
    return Size{(width + scale - 1) / scale, (height + scale - 1) / scale};
}

// tpt_temporal's state across frames (tpt_history).  Declared after the
// DeviceScene it was created from, so that it is destroyed first.
class History {
public:
    History(DeviceScene& scene, int width, int height) {
        tpt_history* h = nullptr;
        check(tpt_history_create(scene.handle(), width, height, &h));
        h_.reset(h);
    }
    void reset() { check(tpt_history_reset(h_.get())); }   // the next temporal() starts over
    // History clipping (tpt_history_set_clip): every later temporal call on this history clamps its
    // reprojected history to the current frame's neighbourhood; nullptr turns it off (the default).
    void setClip(const tpt_clip_params* params) { check(tpt_history_set_clip(h_.get(), params)); }
    tpt_clip_stats clipStats() const {   // of the last temporal call
        tpt_clip_stats st{};
        check(tpt_history_clip_stats(h_.get(), &st));
        return st;
    }
    tpt_history* handle() const { return h_.get(); }

private:
    struct Free {
        void operator()(tpt_history* h) const { tpt_history_destroy(h); }
    };
    std::unique_ptr<tpt_history, Free> h_;
};

// The hosts' defaults of tone mapping (PathTracer::tonemap).  Conventions -- Reinhard's white point
// of 4, the sRGB curve, the photographic key of 0.18 and a 10 % / 95 % trim -- not the result of a sweep.
inline tpt_tonemap_params defaultTonemap() {
    tpt_tonemap_params p{};
    p.op = TPT_TONEMAP_REINHARD;
    p.transfer = TPT_TRANSFER_SRGB;
    p.flags = 0;
    p.ev = 0.0f;
    p.white = 4.0f;
    p.gamma = 2.2f;
    p.key = 0.18f;
    p.p_low = 0.10f;
    p.p_high = 0.95f;
    p.min_ev = -16.0f;
    p.max_ev = 16.0f;
    p.rate = 1.0f;
    return p;
}

// tpt_tonemap's adapted exposure across frames (tpt_exposure).  Declared after the DeviceScene it
// was created from, so that it is destroyed first.
class Exposure {
public:
    explicit Exposure(DeviceScene& scene) {
        tpt_exposure* x = nullptr;
        check(tpt_exposure_create(scene.handle(), &x));
        x_.reset(x);
    }
    void reset() { check(tpt_exposure_reset(x_.get())); }   // the next auto-exposed tonemap() starts at its target
    std::vector<uint64_t> histogram() const {               // of the last auto-exposed call
        std::vector<uint64_t> bins(256);
        check(tpt_exposure_histogram(x_.get(), bins.data()));
        return bins;
    }
    tpt_exposure* handle() const { return x_.get(); }

private:
    struct Free {
        void operator()(tpt_exposure* x) const { tpt_exposure_destroy(x); }
    };
    std::unique_ptr<tpt_exposure, Free> x_;
};

class PathTracer {
public:
    PathTracer() : PathTracer(1920, 1080) {}   // VkEngine default extent (vkEngine.h:24)
    PathTracer(int width, int height, int device = 0) : m_width(width), m_height(height), device_(device) {}
    explicit PathTracer(const EnvLight& env, int width = 1920, int height = 1080, int device = 0)
        : m_width(width), m_height(height), device_(device), envLight(env) {}

    // doTrace (path_tracer.cu:491-554): one frame into a caller framebuffer
    // (host or device pointer, W*H*4 BGRA).  seed 0 -> time(), as the reference.
    // accumulate: progressive rendering (TPT_FLAG_ACCUMULATE) -- continue the
    // previous call's samples for the same frame instead of starting afresh
    // (the reference re-renders fresh samples every frame, vkEngine.cu:244).
    tpt_stats doTrace(DeviceScene& scene, const Camera& camera, uint8_t* framebuffer, int nSamplesPerPixel,
                      uint64_t seed = 0, int max_depth = 8, float* radiance = nullptr,
                      int band_count = 1, int band_index = 0, bool accumulate = false) {
        if (!scene.built()) scene.build();
        tpt_params p{};
        p.width = m_width;
        p.height = m_height;
        p.spp = nSamplesPerPixel;
        p.max_depth = max_depth;
        p.seed = seed ? seed : (accumulate && last_seed_ ? last_seed_ : (uint64_t)std::time(nullptr));
        last_seed_ = p.seed;
        p.band_rows = 16;
        p.band_count = band_count;
        p.band_index = band_index;
        p.flags = accumulate ? TPT_FLAG_ACCUMULATE : 0;
        tpt_stats st{};
        check(tpt_render(scene.handle(), envLight.handle(), &camera.c, &p, radiance, framebuffer, &st));
        return st;
    }

    // A batch of independent frames (seeds[f]) in one trace launch
    // (tpt_render_frames); frame f equals doTrace with seed seeds[f].
    tpt_stats doTraceFrames(DeviceScene& scene, const Camera& camera, const std::vector<uint64_t>& seeds,
                            const std::vector<uint8_t*>& framebuffers, int nSamplesPerPixel, int max_depth = 8,
                            const std::vector<float*>& radiances = {}, int band_count = 1, int band_index = 0) {
        if (!scene.built()) scene.build();
        const size_t n = seeds.size();
        if ((!framebuffers.empty() && framebuffers.size() != n) || (!radiances.empty() && radiances.size() != n))
            throw std::runtime_error("doTraceFrames: need one output buffer per frame");
        tpt_params p{};
        p.width = m_width;
        p.height = m_height;
        p.spp = nSamplesPerPixel;
        p.max_depth = max_depth;
        p.band_rows = 16;
        p.band_count = band_count;
        p.band_index = band_index;
        tpt_stats st{};
        check(tpt_render_frames(scene.handle(), envLight.handle(), &camera.c, &p, (int32_t)n, seeds.data(),
                                radiances.empty() ? nullptr : radiances.data(),
                                framebuffers.empty() ? nullptr : framebuffers.data(), &st));
        return st;
    }

    // Adaptive sampling (tpt_render_adaptive): every 16x16-pixel tile is rendered until its
    // error estimate falls below `target`, from min_spp to at most max_spp = min_spp * 2^j
    // samples; every pixel equals doTrace at its tile's count, bit for bit.  tile_spp /
    // tile_error: nullable, ceil(H / 16) * ceil(W / 16) entries, row 0 = bottom.
    tpt_adaptive_stats doTraceAdaptive(DeviceScene& scene, const Camera& camera, uint8_t* framebuffer, int min_spp,
                                       int max_spp, float target, uint64_t seed = 0, int max_depth = 8,
                                       float* radiance = nullptr, int32_t* tile_spp = nullptr,
                                       float* tile_error = nullptr, int flags = 0) {
        if (!scene.built()) scene.build();
        tpt_params p{};
        p.width = m_width;
        p.height = m_height;
        p.max_depth = max_depth;
        p.seed = seed ? seed : (uint64_t)std::time(nullptr);
        last_seed_ = p.seed;
        p.band_rows = 16;
        p.band_count = 1;
        p.flags = flags;
        tpt_adaptive_params ap{min_spp, max_spp, target, 0};
        tpt_adaptive_stats st{};
        check(tpt_render_adaptive(scene.handle(), envLight.handle(), &camera.c, &p, &ap, radiance, framebuffer,
                                  tile_spp, tile_error, &st));
        return st;
    }

    // First-hit feature buffers of the frame (tpt_render_aov): one ray per pixel
    // centre through the render's traversal.  Every plane is sized and filled;
    // row 0 = bottom, like the radiance.
    AOV renderAOV(DeviceScene& scene, const Camera& camera, double* trace_ms = nullptr) {
        if (!scene.built()) scene.build();
        AOV a;
        a.width = m_width;
        a.height = m_height;
        const size_t n = (size_t)m_width * m_height;
        a.albedo.resize(3 * n);
        a.normal.resize(3 * n);
        a.depth.resize(n);
        a.face.resize(n);
        a.material.resize(n);
        const tpt_aov out = a.view();
        check(tpt_render_aov(scene.handle(), &camera.c, m_width, m_height, &out, trace_ms));
        return a;
    }
    // The same into caller buffers (host or device pointers, each nullable).
    void renderAOV(DeviceScene& scene, const Camera& camera, const tpt_aov& out, double* trace_ms = nullptr) {
        if (!scene.built()) scene.build();
        check(tpt_render_aov(scene.handle(), &camera.c, m_width, m_height, &out, trace_ms));
    }

    // Mirror-path feature buffers (tpt_render_aov_path): renderAOV continued through up to
    // max_bounces perfect mirrors, for denoise / denoiseSVGF and temporalPath (temporal stays on
    // renderAOV's).  bounces (nullable) receives the W*H bounce counts, points (nullable) the
    // W*H*3 terminal points (tpt_render_aov_path_points).
    AOV renderAOVPath(DeviceScene& scene, const Camera& camera, int max_bounces = 8,
                      std::vector<int32_t>* bounces = nullptr, tpt_aov_path_stats* stats = nullptr,
                      std::vector<float>* points = nullptr) {
        AOV a;
        a.width = m_width;
        a.height = m_height;
        const size_t n = (size_t)m_width * m_height;
        a.albedo.resize(3 * n);
        a.normal.resize(3 * n);
        a.depth.resize(n);
        a.face.resize(n);
        a.material.resize(n);
        if (bounces) bounces->resize(n);
        if (points) points->resize(3 * n);
        renderAOVPath(scene, camera, a.view(), bounces ? bounces->data() : nullptr, max_bounces, stats,
                      points ? points->data() : nullptr);
        return a;
    }
    // The same into caller buffers (host or device pointers, each nullable).
    void renderAOVPath(DeviceScene& scene, const Camera& camera, const tpt_aov& out, int32_t* bounces,
                       int max_bounces = 8, tpt_aov_path_stats* stats = nullptr, float* points = nullptr) {
        if (!scene.built()) scene.build();
        const tpt_aov_path_params p{max_bounces, 0};
        check(tpt_render_aov_path_points(scene.handle(), &camera.c, m_width, m_height, &p, &out, bounces, points,
                                         stats));
    }

    // Edge-avoiding a-trous filter (tpt_denoise) of a radiance frame guided by its
    // feature buffers; radiance_out may be radiance_in, framebuffer is written as
    // doTrace writes it (nullable).  Pointers are host or device memory.
    tpt_denoise_stats denoise(DeviceScene& scene, const float* radiance_in, const tpt_aov& guides,
                              float* radiance_out, uint8_t* framebuffer = nullptr,
                              const tpt_denoise_params& params = defaultDenoise(5)) {
        tpt_denoise_stats st{};
        check(tpt_denoise(scene.handle(), m_width, m_height, radiance_in, &guides, &params, radiance_out, framebuffer,
                          &st));
        return st;
    }

    // Temporal reprojection and accumulation (tpt_temporal): this frame's radiance
    // and feature buffers through `history` (of this tracer's frame size), which
    // then holds the frame and `camera`.  radiance_out may be radiance_in; variance
    // and history_len (W*H each) and framebuffer are nullable.  Pointers are host or
    // device memory.
    tpt_temporal_stats temporal(History& history, const Camera& camera, const float* radiance_in,
                                const tpt_aov& guides, float* radiance_out, float* variance = nullptr,
                                float* history_len = nullptr, uint8_t* framebuffer = nullptr,
                                const tpt_temporal_params& params = defaultTemporal()) {
        tpt_temporal_stats st{};
        check(tpt_temporal(history.handle(), &camera.c, radiance_in, &guides, &params, radiance_out, variance,
                           history_len, framebuffer, &st));
        return st;
    }

    // temporal() for a scene whose objects moved since the previous call on `history`
    // (tpt_temporal_motion: setTransforms + build, then this frame's render and feature
    // buffers, `face` included).  motion (W*H*2, nullable) receives each pixel's
    // reprojected minus its own coordinates.
    tpt_temporal_stats temporalMotion(History& history, const Camera& camera, const float* radiance_in,
                                      const tpt_aov& guides, float* radiance_out, float* variance = nullptr,
                                      float* history_len = nullptr, float* motion = nullptr,
                                      uint8_t* framebuffer = nullptr,
                                      const tpt_temporal_params& params = defaultTemporal()) {
        tpt_temporal_stats st{};
        check(tpt_temporal_motion(history.handle(), &camera.c, radiance_in, &guides, &params, radiance_out, variance,
                                  history_len, motion, framebuffer, &st));
        return st;
    }

    // temporal() for a scene whose vertices moved since the previous temporalDeform() on
    // `history` (tpt_temporal_deform: setVertices + build, then this frame's render and feature
    // buffers, `face` included).  The history's scene must be built.  motion as temporalMotion's.
    tpt_temporal_stats temporalDeform(History& history, const Camera& camera, const float* radiance_in,
                                      const tpt_aov& guides, float* radiance_out, float* variance = nullptr,
                                      float* history_len = nullptr, float* motion = nullptr,
                                      uint8_t* framebuffer = nullptr,
                                      const tpt_temporal_params& params = defaultTemporal()) {
        tpt_temporal_stats st{};
        check(tpt_temporal_deform(history.handle(), &camera.c, radiance_in, &guides, &params, radiance_out, variance,
                                  history_len, motion, framebuffer, &st));
        return st;
    }

    // temporal() on mirror-path guides (tpt_temporal_path): renderAOVPath's buffers, bounce counts
    // and terminal points, so that reflections in perfect mirrors keep their history while the
    // camera moves.  Everything else is temporal()'s.
    tpt_temporal_stats temporalPath(History& history, const Camera& camera, const float* radiance_in,
                                    const tpt_aov& path_guides, const int32_t* bounces, const float* points,
                                    float* radiance_out, float* variance = nullptr, float* history_len = nullptr,
                                    uint8_t* framebuffer = nullptr,
                                    const tpt_temporal_path_params& params = defaultTemporalPath()) {
        tpt_temporal_stats st{};
        check(tpt_temporal_path(history.handle(), &camera.c, radiance_in, &path_guides, bounces, points, &params,
                                radiance_out, variance, history_len, framebuffer, &st));
        return st;
    }

    // Variance-guided a-trous filter (tpt_denoise_svgf) of a radiance frame, guided by
    // its feature buffers and by temporal()'s variance and history_len (each nullable:
    // without a variance every pixel takes the spatial estimate).  radiance_out may be
    // radiance_in and variance_out variance_in; variance_out and framebuffer are
    // nullable.  Pointers are host or device memory.
    tpt_svgf_stats denoiseSVGF(DeviceScene& scene, const float* radiance_in, const tpt_aov& guides,
                               const float* variance, const float* history_len, float* radiance_out,
                               float* variance_out = nullptr, uint8_t* framebuffer = nullptr,
                               const tpt_svgf_params& params = defaultSVGF(5)) {
        tpt_svgf_stats st{};
        check(tpt_denoise_svgf(scene.handle(), m_width, m_height, radiance_in, &guides, variance, history_len, &params,
                               radiance_out, variance_out, framebuffer, &st));
        return st;
    }

    // Guided upsampling (tpt_upsample) on the full-size tracer: radiance_low and guides_low are a
    // render of this tracer's camera and its feature buffers at low_width x low_height (a tracer
    // of that size: lowSize), guides the feature buffers at this tracer's size.  radiance_out and
    // framebuffer are nullable, not both.  Pointers are host or device memory.
    tpt_upsample_stats upsample(DeviceScene& scene, int low_width, int low_height, const float* radiance_low,
                                const tpt_aov& guides_low, const tpt_aov& guides, float* radiance_out,
                                uint8_t* framebuffer = nullptr, const tpt_upsample_params& params = defaultUpsample()) {
        tpt_upsample_stats st{};
        check(tpt_upsample(scene.handle(), low_width, low_height, radiance_low, &guides_low, m_width, m_height, &guides,
                           &params, radiance_out, framebuffer, &st));
        return st;
    }

    // The display stage (tpt_tonemap): exposure, tone curve, transfer function and rounding to
    // bytes.  exposure: nullable, carries the adapted value across TPT_TONEMAP_AUTO frames.
    // radiance_out (the mapped colours in [0, 1]; it may be radiance_in) and framebuffer are
    // nullable, not both.  Pointers are host or device memory.
    tpt_tonemap_stats tonemap(DeviceScene& scene, const float* radiance_in, float* radiance_out,
                              uint8_t* framebuffer = nullptr, const tpt_tonemap_params& params = defaultTonemap(),
                              Exposure* exposure = nullptr) {
        tpt_tonemap_stats st{};
        check(tpt_tonemap(scene.handle(), exposure ? exposure->handle() : nullptr, m_width, m_height, radiance_in, &params,
                          radiance_out, framebuffer, &st));
        return st;
    }

    // render(meshFile) (path_tracer.cu:556-579), headless: the reference loops
    // frames in a window; this renders `frames` frames and returns the last --
    // with progressive = true each frame adds its samples to the previous ones.
    Frame render(const std::string& meshFile, int nSamplesPerPixel = 64, uint64_t seed = 0, int max_depth = 8,
                 int frames = 1, bool progressive = false) {
        Scene scene(meshFile, "gltf");
        DeviceScene d = scene.copySceneToDevice(device_);
        d.build();
        Frame f;
        f.width = m_width;
        f.height = m_height;
        f.bgra.assign((size_t)m_width * m_height * 4, 255);
        f.radiance.assign((size_t)m_width * m_height * 3, 0.0f);
        for (int i = 0; i < frames; ++i)
            f.stats = doTrace(d, scene.m_camera, f.bgra.data(), nSamplesPerPixel, seed, max_depth, f.radiance.data(),
                              1, 0, progressive && i > 0);
        return f;
    }

    int m_width, m_height;

private:
    int device_;
    uint64_t last_seed_ = 0;
    EnvLight envLight;
};

}  // namespace tpt
