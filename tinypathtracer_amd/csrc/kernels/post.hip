// post.hip -- what follows a render (DESIGN.md section 5 "Post-pass"): the feature buffers
// (tpt_render_aov, tpt_render_aov_path), the edge-avoiding a-trous wavelet denoiser
// (tpt_denoise; Dammertz et al. 2010), temporal accumulation (tpt_temporal,
// tpt_temporal_motion) and the variance-guided filter (tpt_denoise_svgf; Schied et al. 2017).
//
//  * The steps that several kernels take are written once, ahead of them: the pixel of a
//    lane, the pixel-centre ray, the closest-hit walk, the hit prelude, the feature-buffer
//    write, the albedo floor of (de)modulation, the framebuffer write, the spread counters,
//    the LDS staging of a tile and its halo, the guide terms, the launch shapes.  Their
//    forms (results and the args struct by value, a scalar albedo floor) are the ones under
//    which the kernels' instructions stayed what they were (tools/kernel_diff.py; DESIGN.md
//    section 5 "One text per shared step" has the outcome per kernel).
//  * k_aov / k_aov_path / k_aov_path_points (aov_path_kernel.hpp): one lane per pixel in 16x16 tiles; the ray through the pixel
//    centre walks the render's own closest-hit traversal; k_aov_path follows it through
//    perfect mirrors, a wave looping until none of its lanes continues.  The LDS stack
//    is k_trace_rays'.
//  * k_dn_pack / k_atrous / k_atrous_lds / k_dn_resolve: the filter.  Two float4
//    planes per pixel (colour; normal + depth), one launch per iteration ping-ponging
//    between two colour planes, no atomics.  Each tap is two 16-B loads per lane;
//    a wave of the direct kernel is a 64-pixel row segment, so its lanes read
//    1 KiB of contiguous addresses per plane at every step size.
//  * k_temporal<TILES, Ex...> (temporal_kernel.hpp), a template over the argument structs a variant
//    takes: reprojection and accumulation across frames (tpt_temporal; with MotionArgs
//    tpt_temporal_motion, which follows objects that moved; with TemporalPathArgs tpt_temporal_path,
//    which follows reflections in mirrors; with DeformArgs tpt_temporal_deform, which follows
//    meshes whose vertices moved).
//  * k_clip_box and k_temporal<..., ClipArgs>: history clipping (tpt_history_set_clip): the box
//    of the current frame's colours around each pixel, LDS-staged, and each of the four temporal
//    kernels again with the clamp to it.
//  * k_svgf_pack / k_svgf_estimate / k_svgf_atrous / k_svgf_atrous_lds /
//    k_svgf_resolve: the variance-guided filter (tpt_denoise_svgf) on the same two
//    planes, the variance in the colour plane's fourth component.
//  * k_upsample: guided upsampling (tpt_upsample) of a low-size frame to the full size by the
//    feature buffers of both sizes, one launch, no scratch plane.
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"   // trace_dev.hpp's env helpers, unused here
#include <type_traits>

#include "trace_dev.hpp"

namespace tpt {

// ---- the shared steps ----

// The lane's pixel in 16x16 tiles, each wave an 8x8 sub-tile as in k_trace (primary rays are coherent).
__device__ __forceinline__ int2 tile_wave_xy(int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    return make_int2((int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3));
}

// The ray through the centre of pixel (x, y): sampleRays (path_tracer.cu:42-59), k_trace's
// camera section with the jitter fixed at ju = jv = 0.5, no RNG.  Args: TraceArgs or
// TemporalArgs, which hold the camera under the same names.  Reprojection is exact only
// while the feature buffers' rays and the temporal pass's are the same bits: this is both.
template <class Args>
__device__ __forceinline__ void centre_ray(const Args& a, int x, int y, V3& ro, V3& rd) {
    float lx = 0.5f * 1.0f, lyf = 0.5f * 1.0f;
    lx = lx + (float)x;
    lyf = lyf + (float)y;
    lx = lx * a.inv_w;
    lyf = lyf * a.inv_h;
    lx = lx * a.sensor_w;
    lyf = lyf * a.sensor_h;
    float r4[4];
    mat4_vec4(a.c2w, lx - a.half_sw, lyf - a.half_sh, 0.0f - 1.0f, 0.0f, r4);
    rd = normalize(v3(r4[0], r4[1], r4[2]));
    ro = v3(a.origin[0], a.origin[1], a.origin[2]);
}

// The render's closest hit along (ro, rd), exactly as k_trace_rays mode 1: trav_lane<true>, the
// sliver pass, and the render's grazing-hit rule (trace.hip "Culling"): a grazing hit is traced
// again on the uncull'd binary path.  tg: the ray leaves a surface that it grazes.
__device__ __forceinline__ void closest_hit(Trav& r, const TraceArgs& a, LaneStack<int>& stk, V3 ro, V3 rd, bool tg) {
    uint32_t c_ovf = 0, c_leaf = 0;
    trav_begin(r, ro, rd, TM_CLOSEST, a.boxes_finite != 0, a.emit_root, a.cull_eps, tg);
    trav_lane<true>(r, a, stk, c_ovf);
    if (a.n_sliver_groups > 0) sliver_pass(r, a, c_leaf);
    if (r.fin && r.fid >= 0 && r.mode == TM_CLOSEST && a.graze &&
        grazing(Surf{a.shade[3 * r.fid + 1].w, a.shade[3 * r.fid + 2].w}, r.d)) {
        trav_begin(r, ro, rd, r.mode, a.boxes_finite != 0, a.emit_root, a.cull_eps, true);
        trav_lane<true>(r, a, stk, c_ovf);
    }
}

// The hit prelude (path_tracer.cu:364-374) of the hit r holds: the shading normal, the
// material id (returned), the material's first record (base colour; .w the emission) and the
// face's grazing data.
__device__ __forceinline__ int hit_prelude(const TraceArgs& a, const Trav& r, V3& nrm, float4& m0, Surf& face) {
    const float4* sh = a.shade + 3 * r.fid;
    const float4 s0 = sh[0], s1 = sh[1], s2 = sh[2];
    const float w = 1.0f - r.u - r.v;
    nrm = normalize(((w * v3(s0.x, s0.y, s0.z)) + (r.u * v3(s1.x, s1.y, s1.z))) + (r.v * v3(s2.x, s2.y, s2.z)));
    const int mtl = __float_as_int(s0.w);
    m0 = a.mtl[2 * mtl];
    face = Surf{s1.w, s2.w};
    return mtl;
}

// Pixel p of a plane of three floats per pixel.
__device__ __forceinline__ void store3(float* f, size_t p, V3 v) {
    f[3 * p] = v.x;
    f[3 * p + 1] = v.y;
    f[3 * p + 2] = v.z;
}

// One pixel of the feature buffers, each plane nullable.
__device__ __forceinline__ void write_aov(const AovArgs& o, size_t off, V3 alb, V3 nrm, float depth, int fid, int mtl) {
    if (o.albedo) store3(o.albedo, off, alb);
    if (o.normal) store3(o.normal, off, nrm);
    if (o.depth) o.depth[off] = depth;
    if (o.face) o.face[off] = fid;
    if (o.material) o.material[off] = mtl;
}

// Demodulation divides by max(albedo, kAlbedoFloor), re-modulation multiplies by the same.
constexpr float kAlbedoFloor = 1e-3f;
__device__ __forceinline__ float albedo_floor(float alb) { return fmaxf(alb, kAlbedoFloor); }

// copyToFB's conventions as k_resolve: row 0 = top, B, G, R written, alpha untouched,
// truncating to_uchar.  (x, y): the pixel, row 0 = bottom.
__device__ __forceinline__ void write_bgr(uint8_t* bgra, int width, int height, size_t x, size_t y, V3 c) {
    uint8_t* px = bgra + 4 * (((size_t)height - y - 1) * (size_t)width + x);
    px[0] = to_uchar(c.z);
    px[1] = to_uchar(c.y);
    px[2] = to_uchar(c.x);
}

// The statistics' counters: kTemporalSlots words a cache line apart, a workgroup's chosen by
// its index, added up (or their maximum taken) by the host: every wave of a 1080p frame adding
// to one address would queue 32,400 atomics on it.  spread_count: one integer atomic per wave.
__device__ __forceinline__ unsigned long long* spread_slot(unsigned long long* base) {
    const unsigned slot = ((unsigned)blockIdx.y * gridDim.x + (unsigned)blockIdx.x) % (unsigned)kTemporalSlots;
    return base + (size_t)slot * kTemporalSlotStride;
}
__device__ __forceinline__ void spread_count(unsigned long long* base, int tid, bool counted) {
    const unsigned long long found = __ballot(counted);
    if ((tid & 63) == 0 && found) atomicAdd(spread_slot(base), (unsigned long long)__popcll(found));
}

// tpt_denoise's two guide factors as one exponent: |dn|^2 / sigma_n^2 + dz^2 kz
__device__ __forceinline__ float guide_kz(float z, float sz2) {   // 1 / (sigma_z^2 max(z^2, 1e-12)); finite: a centre tap's 0 * kz is 0
    return fminf(1.0f / (sz2 * fmaxf(z * z, 1e-12f)), kRealMax);
}
__device__ __forceinline__ float guide_arg(float4 gp, float4 gq, float inv_sn2, float kz) {
    const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z, dz = gq.w - gp.w;
    return (nx * nx + ny * ny + nz * nz) * inv_sn2 + (dz * dz) * kz;
}

// A 16x16 tile and its halo staged in LDS as the colour and the guide plane, T pixels a side
// from (x0, y0), zeros outside the frame (never read as a tap, or read at weight 0).  The
// barrier is the caller's.
__device__ __forceinline__ void lds_put(TPT_LDS LdsF4* q, float4 v) {
    q->x = v.x;
    q->y = v.y;
    q->z = v.z;
    q->w = v.w;
}
template <int T, class Args>
__device__ __forceinline__ void stage_tile(TPT_LDS LdsF4* sc, TPT_LDS LdsF4* sg, const Args a, int x0, int y0, int tid) {
    for (int i = tid; i < T * T; i += 256) {
        const int gx = x0 + i % T, gy = y0 + i / T;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = c;
        if (gx >= 0 && gx < a.width && gy >= 0 && gy < a.height) {
            const size_t q = (size_t)gy * (size_t)a.width + (size_t)gx;
            c = a.src[q];
            g = a.guide[q];
        }
        lds_put(sc + i, c);
        lds_put(sg + i, g);
    }
}

// The launch shapes: one lane per pixel in 16x16 tiles (block 256) or in 64-pixel row
// segments (block (64, 4)), or one lane per pixel of the frame as a row of npix.
static dim3 tile_grid(int w, int h) { return dim3((w + 15) / 16, (h + 15) / 16); }
template <class... A>
static hipError_t launch_tiles_or_rows(bool tiles, void (*kt)(A...), size_t lds, void (*kr)(A...), int w, int h,
                                       hipStream_t s, const A&... a) {
    if (tiles) hipLaunchKernelGGL(kt, tile_grid(w, h), dim3(256), lds, s, a...);
    else hipLaunchKernelGGL(kr, dim3((w + 63) / 64, (h + 3) / 4), dim3(64, 4), 0, s, a...);
    return hipGetLastError();
}
template <class Args>
static hipError_t launch_pixels(void (*k)(Args), const Args& a, hipStream_t s) {
    hipLaunchKernelGGL(k, dim3((unsigned)((a.npix + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
// An a-trous iteration: steps 1 and 2 through the LDS-staged kernel ((16 + 4 S)^2 pixels x 32 B) where use_lds.
template <class Args>
static hipError_t launch_filter_step(void (*lds1)(Args), void (*lds2)(Args), void (*direct)(Args), const Args& a,
                                     bool use_lds, hipStream_t s) {
    const int T = 16 + 4 * a.step;
    return launch_tiles_or_rows(use_lds && (a.step == 1 || a.step == 2), a.step == 1 ? lds1 : lds2, (size_t)T * T * 32,
                                direct, a.width, a.height, s, a);
}

// ---- the feature buffers ----

constexpr int kAovLdsSlots = 48;   // LDS stack slots per lane, as k_trace_rays; deeper ones private
constexpr size_t kAovLdsBytes = (size_t)kAovLdsSlots * 256 * sizeof(int);

// tpt_render_aov: the pixel-centre ray's closest hit and its prelude.
__global__ __launch_bounds__(256) void k_aov(TraceArgs a, AovArgs o) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x;
    const int2 xy = tile_wave_xy(tid);
    const int x = xy.x, y = xy.y;
    if (x >= a.width || y >= a.height) return;   // (no barrier below)
    V3 ro, rd;
    centre_ray(a, x, y, ro, rd);
    Trav r;
    LaneStack<int> stk;
    stk.lds = (TPT_LDS int*)lds + tid;
    stk.nlds = kAovLdsSlots;
    closest_hit(r, a, stk, ro, rd, false);   // the camera: no surface
    V3 alb = v3(1.0f, 1.0f, 1.0f), nrm = v3(0.0f, 0.0f, 0.0f);   // miss: demodulation leaves the environment alone
    float depth = 0.0f;
    int mtl = -1;
    if (r.fid >= 0) {
        float4 m0;
        Surf face;
        mtl = hit_prelude(a, r, nrm, m0, face);
        alb = v3(m0.x, m0.y, m0.z);
        depth = r.t;
    }
    write_aov(o, (size_t)x + (size_t)y * (size_t)a.width, alb, nrm, depth, r.fid, mtl);
}

// The mirror-path kernel's text is aov_path_kernel.hpp, compiled twice: as k_aov_path, and with
// TPT_AOV_PATH_POINTS as k_aov_path_points (tpt_render_aov_path_points), which also writes where
// each path ended.  Two compilations of one text, so that k_aov_path's instructions stay what they
// were (tools/kernel_diff.py).
#define TPT_AOV_PATH_POINTS 0
#include "aov_path_kernel.hpp"
#undef TPT_AOV_PATH_POINTS
#define TPT_AOV_PATH_POINTS 1
#include "aov_path_kernel.hpp"
#undef TPT_AOV_PATH_POINTS

hipError_t launch_aov(const TraceArgs& a, const AovArgs& o, hipStream_t s) {
    hipLaunchKernelGGL(k_aov, tile_grid(a.width, a.height), dim3(256), kAovLdsBytes, s, a, o);
    return hipGetLastError();
}

hipError_t launch_aov_path(const TraceArgs& a, const AovArgs& o, const AovPathArgs& p, hipStream_t s) {
    hipLaunchKernelGGL(k_aov_path, tile_grid(a.width, a.height), dim3(256), kAovLdsBytes, s, a, o, p);
    return hipGetLastError();
}

hipError_t launch_aov_path_points(const TraceArgs& a, const AovArgs& o, const AovPathArgs& p, float* points, hipStream_t s) {
    hipLaunchKernelGGL(k_aov_path_points, tile_grid(a.width, a.height), dim3(256), kAovLdsBytes, s, a, o, p, points);
    return hipGetLastError();
}

// ---- the a-trous filter (DESIGN.md section 5 "Post-pass" holds the definition the tests pin) ----

__global__ __launch_bounds__(256) void k_dn_pack(DenoiseArgs a) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.npix) return;
    V3 c = v3(a.radiance_in[3 * p], a.radiance_in[3 * p + 1], a.radiance_in[3 * p + 2]);
    if (a.demodulate)
        c = v3(c.x / albedo_floor(a.albedo[3 * p]), c.y / albedo_floor(a.albedo[3 * p + 1]), c.z / albedo_floor(a.albedo[3 * p + 2]));
    a.color0[p] = make_float4(c.x, c.y, c.z, 0.0f);
    a.guide[p] = make_float4(a.normal[3 * p], a.normal[3 * p + 1], a.normal[3 * p + 2], a.depth[p]);
}

// One pixel's accumulation over its taps.  The weighted mean is kept as
// c(p) + sum w (c(q) - c(p)) / sum w: the same value as sum w c(q) / sum w, and a
// constant image stays constant exactly.  The three edge-stopping exponentials are
// one (their arguments add); exp is the hardware's exp2 of a scaled argument.
struct Taps {
    float4 cp, gp;
    float kz;   // 1 / (sigma_z^2 max(z(p)^2, 1e-12))
    float sw, ar, ag, ab;
    __device__ __forceinline__ void begin(float4 c, float4 g, float sz2) {
        cp = c;
        gp = g;
        kz = guide_kz(g.w, sz2);
        sw = 0.0f;
        ar = ag = ab = 0.0f;
    }
    // (guide_arg's two terms, added one by one to the colour term: guide_arg's own sum would round otherwise)
    __device__ __forceinline__ void tap(float hh, float4 cq, float4 gq, float inv_sc2, float inv_sn2) {
        const float dr = cq.x - cp.x, dg = cq.y - cp.y, db = cq.z - cp.z;
        const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z, dz = gq.w - gp.w;
        const float e = (dr * dr + dg * dg + db * db) * inv_sc2 + (nx * nx + ny * ny + nz * nz) * inv_sn2 +
                        (dz * dz) * kz;
        const float w = hh * __expf(-e);
        sw += w;
        ar += w * dr;
        ag += w * dg;
        ab += w * db;
    }
    __device__ __forceinline__ float4 end() const {
        const float inv = 1.0f / sw;   // the centre tap: sw >= h(0)^2 > 0
        return make_float4(cp.x + ar * inv, cp.y + ag * inv, cp.z + ab * inv, 0.0f);
    }
};

__device__ __forceinline__ float atrous_h(int d) {   // [1/16, 1/4, 3/8, 1/4, 1/16]
    return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

// Direct version: every tap from global memory (L1 / L2).  Block (64, 4).
__global__ __launch_bounds__(256) void k_atrous(AtrousArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y * 4 + (int)threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    Taps t;
    t.begin(a.src[p], a.guide[p], a.sz2);
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.height) continue;
        const size_t row = (size_t)qy * (size_t)a.width;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.width) continue;
            t.tap(atrous_h(dx) * atrous_h(dy), a.src[row + qx], a.guide[row + qx], a.inv_sc2, a.inv_sn2);
        }
    }
    a.dst[p] = t.end();
}

// LDS version for steps 1 and 2: a 16x16 tile and its halo of 2 S pixels staged once
// ((16 + 4 S)^2 pixels x 32 B: 12.5 KB at S = 1, 18 KB at S = 2), every tap an LDS
// read.  The same taps in the same order as k_atrous: bit-identical output.
template <int S>
__global__ __launch_bounds__(256) void k_atrous_lds(AtrousArgs a) {
    constexpr int T = 16 + 4 * S;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    TPT_LDS LdsF4* sc = (TPT_LDS LdsF4*)lds;
    TPT_LDS LdsF4* sg = sc + T * T;
    const int tid = threadIdx.x;
    const int x0 = (int)blockIdx.x * 16 - 2 * S, y0 = (int)blockIdx.y * 16 - 2 * S;
    stage_tile<T>(sc, sg, a, x0, y0, tid);
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    const int x = (int)blockIdx.x * 16 + tx, y = (int)blockIdx.y * 16 + ty;
    if (x >= a.width || y >= a.height) return;
    const int c0 = (ty + 2 * S) * T + tx + 2 * S;
    Taps t;
    t.begin(lds_f4(sc + c0), lds_f4(sg + c0), a.sz2);
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * S;
        if (qy < 0 || qy >= a.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * S;
            if (qx < 0 || qx >= a.width) continue;
            const int q = c0 + dy * S * T + dx * S;
            t.tap(atrous_h(dx) * atrous_h(dy), lds_f4(sc + q), lds_f4(sg + q), a.inv_sc2, a.inv_sn2);
        }
    }
    a.dst[(size_t)y * (size_t)a.width + (size_t)x] = t.end();
}

// Re-modulation, the radiance readout and the framebuffer (write_bgr).
__global__ __launch_bounds__(256) void k_dn_resolve(DenoiseArgs a) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.npix) return;
    const float4 c4 = a.color0[p];
    V3 c = v3(c4.x, c4.y, c4.z);
    if (a.demodulate)
        c = v3(c.x * albedo_floor(a.albedo[3 * p]), c.y * albedo_floor(a.albedo[3 * p + 1]), c.z * albedo_floor(a.albedo[3 * p + 2]));
    if (a.radiance_out) store3(a.radiance_out, p, c);
    if (a.bgra) {
        const size_t y = p / (size_t)a.width;
        write_bgr(a.bgra, a.width, a.height, p - y * (size_t)a.width, y, c);
    }
}

hipError_t launch_denoise_pack(const DenoiseArgs& a, hipStream_t s) { return launch_pixels(k_dn_pack, a, s); }
hipError_t launch_atrous(const AtrousArgs& a, bool use_lds, hipStream_t s) {
    return launch_filter_step(k_atrous_lds<1>, k_atrous_lds<2>, k_atrous, a, use_lds, s);
}
hipError_t launch_denoise_resolve(const DenoiseArgs& a, hipStream_t s) { return launch_pixels(k_dn_resolve, a, s); }

// ---- temporal reprojection and accumulation (DESIGN.md section 5 "Post-pass" holds the definition) ----

constexpr float kSnap = 1.0f / 1024.0f;      // a reprojected coordinate this close to a pixel centre is that centre
constexpr float kMinWsum = 1.0f / 16.0f;     // least sum of valid bilinear weights that counts as history

// k_temporal<TILES, Ex...> (temporal_kernel.hpp) is one template for the eight temporal kernels: the
// pack Ex holds the argument structs a variant takes on top of TemporalArgs, so each instantiation
// has the parameter list and the kernarg layout of the kernel it replaces, and its additions are the
// `if constexpr` blocks there.  Its lane's pixel, ray, albedo floor, framebuffer write and counter are
// the shared steps above.  The kernels used to be eight compilations of that text under four macros,
// because a bool template parameter had reordered k_temporal's instructions.  What allowed the
// template (tools/kernel_diff.py @tools/kernel_diff_temporal.args, device-only builds of this file at
// the commit before and here): "identical: 37; different: 0", the sixteen temporal kernels among
// them, with the registers, scratch and occupancy they had (make resource-usage-post).
#include "temporal_kernel.hpp"

// The box of history clipping (DESIGN.md section 5 "History clipping" holds the definition):
// 16x16 tiles; per pixel, the first two moments of the colour the temporal kernel accumulates
// over the taps of the (2 R + 1)^2 window that are similar to the centre -- the same material
// (and bounce count, PATH), and on a hit a depth within depth_tol of the centre's and a normal
// with n(q) . n(p) >= normal_min -- taken about the centre's colour as k_svgf_estimate takes its:
// exactly 0 variance on a constant window.  The tile and its halo of R pixels are staged in LDS
// once per staged pixel as (c.rgb, bits(m)) and (n.xyz, z), PATH: and k; the demodulating
// divisions are made there, not once per tap.  (16 + 2 R)^2 x 32 B (PATH: 36 B): 17.4 KB at most.
// Halo pixels outside the frame are zero-filled and excluded by the in-frame predicate.  Fewer than
// four taps give no box: lo = -inf, hi = +inf.
template <int R, bool PATH>
__global__ __launch_bounds__(256) void k_clip_box(ClipBoxArgs a) {
    constexpr int T = 16 + 2 * R;
    __shared__ LdsF4 sc_[T * T];
    __shared__ LdsF4 sg_[T * T];
    __shared__ int sk[PATH ? T * T : 1];
    TPT_LDS LdsF4* sc = (TPT_LDS LdsF4*)sc_;
    TPT_LDS LdsF4* sg = (TPT_LDS LdsF4*)sg_;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int x0 = (int)blockIdx.x * 16 - R, y0 = (int)blockIdx.y * 16 - R;
    // Two rounds of 256 staged pixels (T * T <= 484).  The loads of both are issued before the first is
    // used: a staged pixel outside the frame, or past the tile, reads pixel 0 and is not kept, so no
    // load waits behind a branch (the second round, which fills a quarter of the lanes at R = 1,
    // otherwise starts only after the first round's LDS stores).
    constexpr int ROUNDS = (T * T + 255) / 256;
    static_assert(ROUNDS == 2, "k_clip_box stages its tile in two rounds");
    bool in[ROUNDS];
    V3 rad[ROUNDS], alb[ROUNDS], nrm[ROUNDS];
    float z[ROUNDS];
    int m[ROUNDS], k[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int i = tid + 256 * r;
        const int gx = x0 + i % T, gy = y0 + i / T;
        in[r] = i < T * T && gx >= 0 && gx < a.width && gy >= 0 && gy < a.height;
        const size_t q = in[r] ? (size_t)gy * (size_t)a.width + (size_t)gx : 0;
        rad[r] = v3(a.radiance_in[3 * q], a.radiance_in[3 * q + 1], a.radiance_in[3 * q + 2]);
        alb[r] = v3(1.0f, 1.0f, 1.0f);
        if (a.demodulate) alb[r] = v3(a.albedo[3 * q], a.albedo[3 * q + 1], a.albedo[3 * q + 2]);
        nrm[r] = v3(a.normal[3 * q], a.normal[3 * q + 1], a.normal[3 * q + 2]);
        z[r] = a.depth[q];
        m[r] = a.material[q];
        k[r] = PATH ? a.bounces[q] : 0;
    }
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int i = tid + 256 * r;
        if (i >= T * T) continue;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = c;
        if (in[r]) {
            V3 cc = rad[r];
            if (a.demodulate)   // k_temporal's arithmetic
                cc = v3(cc.x / albedo_floor(alb[r].x), cc.y / albedo_floor(alb[r].y), cc.z / albedo_floor(alb[r].z));
            c = make_float4(cc.x, cc.y, cc.z, __int_as_float(m[r]));
            g = make_float4(nrm[r].x, nrm[r].y, nrm[r].z, z[r]);
        }
        lds_put(sc + i, c);
        lds_put(sg + i, g);
        if (PATH) sk[i] = in[r] ? k[r] : 0;
    }
    __syncthreads();
    const int x = (int)blockIdx.x * 16 + tx, y = (int)blockIdx.y * 16 + ty;
    const bool inside = x < a.width && y < a.height;
    bool boxed = false;
    if (inside) {
        const int c0 = (ty + R) * T + tx + R;
        const float4 cp = lds_f4(sc + c0), gp = lds_f4(sg + c0);
        const int mp = __float_as_int(cp.w);
        const int kp = PATH ? sk[c0] : 0;
        const bool hit = mp >= 0;
        const float ztol = a.depth_tol * gp.w;
        float n = 0.0f;
        float s1x = 0.0f, s1y = 0.0f, s1z = 0.0f, s2x = 0.0f, s2y = 0.0f, s2z = 0.0f;
#pragma unroll
        for (int dy = -R; dy <= R; ++dy) {
            const bool row_in = y + dy >= 0 && y + dy < a.height;
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int q = c0 + dy * T + dx;
                const float4 cq = lds_f4(sc + q), gq = lds_f4(sg + q);
                bool ok = row_in && x + dx >= 0 && x + dx < a.width && __float_as_int(cq.w) == mp;
                if (PATH) ok = ok && sk[q] == kp;
                if (hit) ok = ok && fabsf(gq.w - gp.w) <= ztol && (gq.x * gp.x + gq.y * gp.y) + gq.z * gp.z >= a.normal_min;
                if (dx == 0 && dy == 0) ok = true;   // the centre always counts
                if (!ok) continue;
                const float ex = cq.x - cp.x, ey = cq.y - cp.y, ez = cq.z - cp.z;
                n += 1.0f;
                s1x += ex;
                s1y += ey;
                s1z += ez;
                s2x += ex * ex;
                s2y += ey * ey;
                s2z += ez * ez;
            }
        }
        float4 lo = make_float4(-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), n);
        float4 hi = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), 0.0f);
        boxed = n >= 4.0f;
        if (boxed) {
            const float mx = s1x / n, my = s1y / n, mz = s1z / n;
            const float gx = a.gamma * fsqrt(fmaxf(s2x / n - mx * mx, 0.0f));
            const float gy = a.gamma * fsqrt(fmaxf(s2y / n - my * my, 0.0f));
            const float gz = a.gamma * fsqrt(fmaxf(s2z / n - mz * mz, 0.0f));
            const float ux = cp.x + mx, uy = cp.y + my, uz = cp.z + mz;
            lo = make_float4(ux - gx, uy - gy, uz - gz, n);
            hi = make_float4(ux + gx, uy + gy, uz + gz, 0.0f);
        }
        const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
        a.lo[p] = lo;
        a.hi[p] = hi;
    }
    spread_count(a.boxed, tid, boxed);   // the statistic
}

template <int R>
static hipError_t launch_clip_box_r(const ClipBoxArgs& a, hipStream_t s) {
    if (a.bounces) hipLaunchKernelGGL((k_clip_box<R, true>), tile_grid(a.width, a.height), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_clip_box<R, false>), tile_grid(a.width, a.height), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_clip_box(const ClipBoxArgs& a, hipStream_t s) {
    switch (a.radius) {
        case 1: return launch_clip_box_r<1>(a, s);
        case 2: return launch_clip_box_r<2>(a, s);
        case 3: return launch_clip_box_r<3>(a, s);
        default: return hipErrorInvalidValue;   // (tpt_history_set_clip refuses every other radius)
    }
}

template <class... Ex>
static hipError_t launch_temporal_as(const TemporalArgs& a, hipStream_t s, const Ex&... ex) {
    return launch_tiles_or_rows(a.tiles != 0, k_temporal<true, Ex...>, 0, k_temporal<false, Ex...>, a.width, a.height, s, a, ex...);
}
hipError_t launch_temporal(const TemporalArgs& a, const MotionArgs* mo, const TemporalPathArgs* pa, const DeformArgs* de,
                           const ClipArgs* cl, hipStream_t s) {
    if ((mo != nullptr) + (pa != nullptr) + (de != nullptr) > 1) return hipErrorInvalidValue;
    const auto clip_or_not = [&](const auto&... kind) {
        return cl ? launch_temporal_as(a, s, kind..., *cl) : launch_temporal_as(a, s, kind...);
    };
    return mo ? clip_or_not(*mo) : pa ? clip_or_not(*pa) : de ? clip_or_not(*de) : clip_or_not();
}

// ---- the variance-guided a-trous filter (Schied et al. 2017; DESIGN.md section 5 "Post-pass" holds the definition) ----
//
// tpt_denoise's two float4 planes per pixel, the colour plane's fourth component
// carrying the variance of the luminance: a tap is still two 16-B loads, and the
// variance is filtered without memory traffic of its own.  Pack, the spatial variance
// estimate of the pixels with a short history (plane 0 -> plane 1), one launch per
// iteration between the two colour planes, resolve.  A tap outside the frame is not
// skipped by a branch but given the weight 0, its loads sent to the lane's own pixel
// (the LDS variant reads its zero-filled halo): the same sums, and a row's loads are
// unconditional, so they are issued together ahead of their use.

__device__ __forceinline__ float svgf_lum(float r, float g, float b) {   // k_temporal's L
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}

__global__ __launch_bounds__(256) void k_svgf_pack(SvgfArgs a) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.npix) return;
    V3 c = v3(a.radiance_in[3 * p], a.radiance_in[3 * p + 1], a.radiance_in[3 * p + 2]);
    if (a.demodulate)
        c = v3(c.x / albedo_floor(a.albedo[3 * p]), c.y / albedo_floor(a.albedo[3 * p + 1]), c.z / albedo_floor(a.albedo[3 * p + 2]));
    const float v = a.variance_in ? fmaxf(a.variance_in[p], 0.0f) : 0.0f;
    a.dst[p] = make_float4(c.x, c.y, c.z, v);
    a.guide[p] = make_float4(a.normal[3 * p], a.normal[3 * p + 1], a.normal[3 * p + 2], a.depth[p]);
}

// The spatial estimate: 16x16 tiles; a pixel with N < min_history replaces its
// variance by that of L over its 7x7 window under the guide weight, times min_history
// / N; every other pixel is copied.  The tile and its halo of 3 pixels are staged in
// LDS as the luminance and the guide (22^2 x 20 B = 9.5 KB: L is computed once per
// staged pixel, not once per tap), and only short lanes walk the 49 taps.  A block
// without a short pixel copies its pixels and leaves before staging anything.  The
// moments are taken about the centre's luminance: the same variance, without the
// cancellation of mu2 - mu1^2 at a large mean, and exactly 0 on a constant window.
__global__ __launch_bounds__(256) void k_svgf_estimate(SvgfArgs a) {
    constexpr int T = 16 + 2 * 3;
    __shared__ float sl[T * T];
    __shared__ LdsF4 sg_[T * T];
    TPT_LDS LdsF4* sg = (TPT_LDS LdsF4*)sg_;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int x = (int)blockIdx.x * 16 + tx, y = (int)blockIdx.y * 16 + ty;
    const bool inside = x < a.width && y < a.height;
    const size_t p = inside ? (size_t)y * (size_t)a.width + (size_t)x : 0;
    float N = 1.0f;
    bool is_short = false;
    if (inside) {
        if (!a.variance_in) is_short = true;
        else if (a.history_len) {
            N = fmaxf(a.history_len[p], 1.0f);
            is_short = N < a.min_history;
        }
    }
    spread_count(a.estimated, tid, is_short);   // the statistic
    if (!__syncthreads_or(is_short ? 1 : 0)) {
        if (inside) a.dst[p] = a.src[p];
        return;
    }
    const int x0 = (int)blockIdx.x * 16 - 3, y0 = (int)blockIdx.y * 16 - 3;
    for (int i = tid; i < T * T; i += 256) {
        const int gx = x0 + i % T, gy = y0 + i / T;
        float l = 0.0f;
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gx >= 0 && gx < a.width && gy >= 0 && gy < a.height) {   // (outside the frame: weight 0 below)
            const size_t q = (size_t)gy * (size_t)a.width + (size_t)gx;
            const float4 c = a.src[q];
            l = svgf_lum(c.x, c.y, c.z);
            g = a.guide[q];
        }
        sl[i] = l;
        sg[i].x = g.x;
        sg[i].y = g.y;
        sg[i].z = g.z;
        sg[i].w = g.w;
    }
    __syncthreads();
    if (!inside) return;
    float4 c = a.src[p];
    if (is_short) {
        const int c0 = (ty + 3) * T + tx + 3;
        const float lp = sl[c0];
        const float4 gp = lds_f4(sg + c0);
        const float kz = guide_kz(gp.w, a.sz2);
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int dy = -3; dy <= 3; ++dy) {
            const bool row_in = y + dy >= 0 && y + dy < a.height;
#pragma unroll
            for (int dx = -3; dx <= 3; ++dx) {
                const bool in = row_in && x + dx >= 0 && x + dx < a.width;
                const int q = c0 + dy * T + dx;
                const float d = sl[q] - lp;
                const float w = in ? __expf(-guide_arg(gp, lds_f4(sg + q), a.inv_sn2, kz)) : 0.0f;
                s0 += w;
                s1 += w * d;
                s2 += w * (d * d);
            }
        }
        const float m1 = s1 / s0, m2 = s2 / s0;   // the centre tap: s0 >= 1
        c.w = fmaxf(m2 - m1 * m1, 0.0f) * (a.min_history / N);
    }
    a.dst[p] = c;
}

// One pixel's accumulation over its taps, as Taps: the mean kept as c(p) + sum w dc /
// sum w, one exponential per tap.  The luminance factor's scale comes from the
// prefiltered variance at p; the variance summed is the unprefiltered one at q.
struct SvgfTaps {
    float4 cp, gp;
    float lp, kl, kz;   // L(c(p)); 1 / (sigma_l sqrt(vbar + 1e-10)); 1 / (sigma_z^2 max(z(p)^2, 1e-12))
    float sw, ar, ag, ab, av;
    __device__ __forceinline__ void begin(float4 c, float4 g, float vbar, float sigma_lum, float sz2) {
        cp = c;
        gp = g;
        lp = svgf_lum(c.x, c.y, c.z);
        kl = fminf(1.0f / (sigma_lum * fsqrt(vbar + 1e-10f)), kRealMax);   // (finite: the centre tap's 0 * kl is 0)
        kz = guide_kz(g.w, sz2);
        sw = 0.0f;
        ar = ag = ab = av = 0.0f;
    }
    // hh: h(dx) h(dy), or 0 for a tap outside the frame (cq, gq then hold any finite values)
    __device__ __forceinline__ void tap(float hh, float4 cq, float4 gq, float inv_sn2) {
        const float dr = cq.x - cp.x, dg = cq.y - cp.y, db = cq.z - cp.z;
        const float e = fabsf(svgf_lum(cq.x, cq.y, cq.z) - lp) * kl + guide_arg(gp, gq, inv_sn2, kz);
        const float w = hh * __expf(-e);
        sw += w;
        ar += w * dr;
        ag += w * dg;
        ab += w * db;
        av += (w * w) * cq.w;
    }
    __device__ __forceinline__ float4 end() const {
        const float inv = 1.0f / sw;   // the centre tap: sw >= h(0)^2 > 0
        return make_float4(cp.x + ar * inv, cp.y + ag * inv, cp.z + ab * inv, av * (inv * inv));
    }
};

// The 3x3 binomial prefilter of the variance, g = [1/4, 1/2, 1/4], over the taps inside
// the frame (bit k = 3 (dy + 1) + dx + 1 of `in`).  Both filter kernels call it with
// the same nine values.
__device__ __forceinline__ float svgf_prefilter(const float (&v)[9], unsigned in) {
    float s = 0.0f, sw = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float g = (k / 3 == 1 ? 0.5f : 0.25f) * (k % 3 == 1 ? 0.5f : 0.25f);
        const float w = ((in >> k) & 1u) ? g : 0.0f;
        s += w * v[k];
        sw += w;
    }
    return s / sw;   // the centre: sw >= 1/4
}

// Direct version: every tap from global memory (L1 / L2).  Block (64, 4), a wave a
// 64-pixel row segment as k_atrous.  The eight prefilter taps around p read the .w
// words only.  A row's ten loads are issued before its five taps are summed.
__global__ __launch_bounds__(256) void k_svgf_atrous(SvgfFilterArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y * 4 + (int)threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const float4 cp = a.src[p], gp = a.guide[p];
    const float* vw = (const float*)a.src + 3;
    float v9[9];
    unsigned in9 = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int k = 3 * (dy + 1) + dx + 1;
            const int qx = x + dx, qy = y + dy;
            const bool in = qx >= 0 && qx < a.width && qy >= 0 && qy < a.height;
            const size_t q = in ? (size_t)qy * (size_t)a.width + (size_t)qx : p;
            v9[k] = (dx == 0 && dy == 0) ? cp.w : vw[4 * q];
            in9 |= in ? 1u << k : 0u;
        }
    SvgfTaps t;
    t.begin(cp, gp, svgf_prefilter(v9, in9), a.sigma_lum, a.sz2);
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * a.step;
        const bool row_in = qy >= 0 && qy < a.height;
        const size_t row = (size_t)(row_in ? qy : y) * (size_t)a.width;
        float4 cq[5], gq[5];
        float hh[5];
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * a.step;
            const bool in = row_in && qx >= 0 && qx < a.width;
            const size_t q = in ? row + (size_t)qx : p;
            cq[dx + 2] = a.src[q];
            gq[dx + 2] = a.guide[q];
            hh[dx + 2] = in ? atrous_h(dx) * atrous_h(dy) : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) t.tap(hh[k], cq[k], gq[k], a.inv_sn2);
    }
    a.dst[p] = t.end();
}

// LDS version for steps 1 and 2, as k_atrous_lds: a 16x16 tile and its halo of 2 S
// pixels staged once, zero-filled outside the frame; the halo holds the prefilter's
// taps too.  The same taps in the same order as k_svgf_atrous: bit-identical output.
template <int S>
__global__ __launch_bounds__(256) void k_svgf_atrous_lds(SvgfFilterArgs a) {
    constexpr int T = 16 + 4 * S;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    TPT_LDS LdsF4* sc = (TPT_LDS LdsF4*)lds;
    TPT_LDS LdsF4* sg = sc + T * T;
    const int tid = threadIdx.x;
    const int x0 = (int)blockIdx.x * 16 - 2 * S, y0 = (int)blockIdx.y * 16 - 2 * S;
    stage_tile<T>(sc, sg, a, x0, y0, tid);
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    const int x = (int)blockIdx.x * 16 + tx, y = (int)blockIdx.y * 16 + ty;
    if (x >= a.width || y >= a.height) return;
    const int c0 = (ty + 2 * S) * T + tx + 2 * S;
    const float4 cp = lds_f4(sc + c0);
    float v9[9];
    unsigned in9 = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int k = 3 * (dy + 1) + dx + 1;
            const int qx = x + dx, qy = y + dy;
            const bool in = qx >= 0 && qx < a.width && qy >= 0 && qy < a.height;
            v9[k] = (dx == 0 && dy == 0) ? cp.w : sc[c0 + dy * T + dx].w;
            in9 |= in ? 1u << k : 0u;
        }
    SvgfTaps t;
    t.begin(cp, lds_f4(sg + c0), svgf_prefilter(v9, in9), a.sigma_lum, a.sz2);
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * S;
        const bool row_in = qy >= 0 && qy < a.height;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * S;
            const bool in = row_in && qx >= 0 && qx < a.width;
            const int q = c0 + dy * S * T + dx * S;
            t.tap(in ? atrous_h(dx) * atrous_h(dy) : 0.0f, lds_f4(sc + q), lds_f4(sg + q), a.inv_sn2);
        }
    }
    a.dst[(size_t)y * (size_t)a.width + (size_t)x] = t.end();
}

// Re-modulation and the outputs, as k_dn_resolve; passthrough
// (iterations 0): the radiance is the input bit for bit.
__global__ __launch_bounds__(256) void k_svgf_resolve(SvgfArgs a) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.npix) return;
    const float4 c4 = a.src[p];
    float r = c4.x, g = c4.y, b = c4.z;
    if (a.passthrough) {
        r = a.radiance_in[3 * p];
        g = a.radiance_in[3 * p + 1];
        b = a.radiance_in[3 * p + 2];
    } else if (a.demodulate) {
        r = r * albedo_floor(a.albedo[3 * p]);
        g = g * albedo_floor(a.albedo[3 * p + 1]);
        b = b * albedo_floor(a.albedo[3 * p + 2]);
    }
    const V3 c = v3(r, g, b);
    if (a.radiance_out) store3(a.radiance_out, p, c);
    if (a.variance_out) a.variance_out[p] = c4.w;
    if (a.bgra) {
        const size_t y = p / (size_t)a.width;
        write_bgr(a.bgra, a.width, a.height, p - y * (size_t)a.width, y, c);
    }
}

hipError_t launch_svgf_pack(const SvgfArgs& a, hipStream_t s) { return launch_pixels(k_svgf_pack, a, s); }
hipError_t launch_svgf_estimate(const SvgfArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_svgf_estimate, tile_grid(a.width, a.height), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_svgf_filter(const SvgfFilterArgs& a, bool use_lds, hipStream_t s) {
    return launch_filter_step(k_svgf_atrous_lds<1>, k_svgf_atrous_lds<2>, k_svgf_atrous, a, use_lds, s);
}
hipError_t launch_svgf_resolve(const SvgfArgs& a, hipStream_t s) { return launch_pixels(k_svgf_resolve, a, s); }

// ---- guided upsampling (tpt_upsample; DESIGN.md section 5 "Guided upsampling" holds the definition) ----

// One axis of a full-size pixel's footprint in the low frame, in integers: n = (2 x + 1) lo - full,
// q0 = floor(n / 2 full), r = n - 2 full q0, f = r / 2 full.  n + 2 full > 0, so the floor is an
// unsigned division of that.  q[0], q[1]: the two taps' coordinates, clamped; r == 0: the second
// has the weight 0 and is no tap.
struct UpAxis {
    int q[2];
    float f;
    bool two;
};
__device__ __forceinline__ UpAxis up_axis(int x, int lo, int full) {
    const unsigned long long d = 2ull * (unsigned long long)full;
    const unsigned long long n = (2ull * (unsigned long long)x + 1ull) * (unsigned long long)lo + (unsigned long long)full;
    const int q0 = (int)(n / d) - 1;   // -1 .. lo - 1
    const unsigned long long r = n % d;
    UpAxis ax;
    ax.q[0] = q0 < 0 ? 0 : q0;
    ax.q[1] = q0 + 1 > lo - 1 ? lo - 1 : q0 + 1;
    ax.f = (float)r / (float)d;
    ax.two = r != 0;
    return ax;
}

// One lane per full-size pixel, a wave a 64-pixel row segment (block (64, 4)): its reads of the
// full-size guides and its 12-B writes are contiguous.  The four taps' low-size planes are read
// as they are (no pack step: at scale s each low pixel is a tap of about 4 s^2 lanes, nearly all
// of them in the same or the neighbouring wave, so the gathers are L1 / L2 hits), every load of
// a tap issued before the first is used, a tap of weight 0 included (its address is a clamped
// neighbour's).  No LDS, no floating-point atomics.
__global__ __launch_bounds__(256) void k_upsample(UpsampleArgs a) {
    const int tid = (int)threadIdx.y * 64 + (int)threadIdx.x;
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y * 4 + (int)threadIdx.y;
    bool fallback = false;
    if (x < a.width && y < a.height) {
        const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
        const UpAxis ax = up_axis(x, a.low_width, a.width), ay = up_axis(y, a.low_height, a.height);
        const int mp = a.material[p];
        const float4 gp = make_float4(a.normal[3 * p], a.normal[3 * p + 1], a.normal[3 * p + 2], a.depth[p]);
        V3 albp = v3(1.0f, 1.0f, 1.0f);
        if (a.demodulate) albp = v3(a.albedo[3 * p], a.albedo[3 * p + 1], a.albedo[3 * p + 2]);
        V3 c[4], alb[4];
        float4 g[4];
        int m[4];
        float b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // (0,0), (1,0), (0,1), (1,1)
            const int i = k & 1, j = k >> 1;
            const size_t q = (size_t)ay.q[j] * (size_t)a.low_width + (size_t)ax.q[i];
            c[k] = v3(a.radiance_low[3 * q], a.radiance_low[3 * q + 1], a.radiance_low[3 * q + 2]);
            g[k] = make_float4(a.normal_low[3 * q], a.normal_low[3 * q + 1], a.normal_low[3 * q + 2], a.depth_low[q]);
            m[k] = a.material_low[q];
            alb[k] = v3(1.0f, 1.0f, 1.0f);
            if (a.demodulate) alb[k] = v3(a.albedo_low[3 * q], a.albedo_low[3 * q + 1], a.albedo_low[3 * q + 2]);
            // the bilinear weight; a tap of weight 0 is known from the integer remainder
            const bool tap = (i == 0 || ax.two) && (j == 0 || ay.two);
            b[k] = tap ? (i ? ax.f : 1.0f - ax.f) * (j ? ay.f : 1.0f - ay.f) : 0.0f;
        }
        const float kz = guide_kz(gp.w, a.sz2);
        float e[4], emin = kRealMax;
        bool ok[4], any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ok[k] = b[k] > 0.0f && m[k] == mp;
            e[k] = fminf(guide_arg(gp, g[k], a.inv_sn2, kz), kRealMax);
            if (ok[k]) emin = fminf(emin, e[k]);
            any = any || ok[k];
        }
        fallback = !any;
        // accepted taps: the edge-weighted mean of the (demodulated) colours; none: the bilinear
        // mean of the radiance as given.  Both as c_r + sum w (c_q - c_r) / sum w about the first
        // tap that counts: a constant stays constant exactly.
        const bool demod = a.demodulate && any;
        V3 cr = v3(0.0f, 0.0f, 0.0f);
        bool first = true;
        float sw = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool counts = any ? ok[k] : b[k] > 0.0f;
            if (!counts) continue;
            V3 cq = c[k];
            if (demod) cq = v3(cq.x / albedo_floor(alb[k].x), cq.y / albedo_floor(alb[k].y), cq.z / albedo_floor(alb[k].z));
            if (first) cr = cq;
            first = false;
            const float w = any ? b[k] * __expf(-(e[k] - emin)) : b[k];
            sw += w;
            ar += w * (cq.x - cr.x);
            ag += w * (cq.y - cr.y);
            ab += w * (cq.z - cr.z);
        }
        const float inv = 1.0f / sw;   // sw >= the weight b > 0 of the tap with e = emin, or of tap (0, 0)
        V3 o = v3(cr.x + ar * inv, cr.y + ag * inv, cr.z + ab * inv);
        if (demod) o = v3(o.x * albedo_floor(albp.x), o.y * albedo_floor(albp.y), o.z * albedo_floor(albp.z));
        if (a.radiance_out) store3(a.radiance_out, p, o);
        if (a.bgra) write_bgr(a.bgra, a.width, a.height, (size_t)x, (size_t)y, o);
    }
    spread_count(a.fallback, tid, fallback);   // the statistic
}

hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t s) {
    return launch_tiles_or_rows(false, k_upsample, 0, k_upsample, a.width, a.height, s, a);
}

}  // namespace tpt
