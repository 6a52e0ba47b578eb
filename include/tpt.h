/*
 * tpt.h -- C-ABI of the MI355X-native TinyPathTracer hot path (libtpt.so).
 *
 * Drop-in boundary for the reference's render job
 *   PathTracer::doTrace(DeviceScene&, Camera&, unsigned char* fb, int spp)
 *   (include/path_tracer.h:34, src/path_tracer.cu:491-554)
 * and for the device ABI of its `trace` kernel
 *   (src/path_tracer.cu:296-299).  Plain pointers and sizes only; no
 * exceptions cross this boundary (errors: tpt_status + tpt_last_error()).
 *
 * Handles own device memory; caller buffers are borrowed.  A tpt_scene lives
 * on one HIP device (a device may hold any number of scenes); calls on
 * different scenes may run concurrently from different host threads, calls on
 * one scene -- and on the histories made from it -- must be serialised by the
 * caller.  A const tpt_env* is read-only after its creation and may be shared
 * by concurrent renders of different scenes; destroy it once they have
 * returned.  tpt_last_error() is per thread: it returns the message of the
 * calling thread's last failed call, valid until that thread's next one.
 */
#ifndef TPT_H
#define TPT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPT_VERSION_MAJOR 0
#define TPT_VERSION_MINOR 1

typedef enum {
    TPT_OK = 0,
    TPT_ERR_INVALID_ARG = 1,
    TPT_ERR_HIP = 2,
    TPT_ERR_OOM = 3,
    TPT_ERR_IO = 4,
    TPT_ERR_PARSE = 5,
    TPT_ERR_NO_DEVICE = 6
} tpt_status;

/* Material, 60 bytes: the reference's Material (include/material.h:86-120). */
typedef struct {
    float base_color[3];
    float emission_factor;
    float eta;
    float metallic;
    float subsurface, specular, roughness, specular_tint, anisotropic,
          sheen, sheen_tint, clearcoat, clearcoat_gloss;
} tpt_material;

/* DeltaLight flattened (include/delta_light.h:35-130); type 0 point,
 * 1 directional, 2 spot.  Intensities already in the reference's units
 * (point/spot lumens x 1/683, mesh.cu:276,290). */
typedef struct {
    int32_t type;
    float color[3];
    float intensity;
    float pos[3];
    float direction[3];
    float cos_outer;
    float inv_cos_cone_diff;
} tpt_light;

/* MtlInterval (include/mesh.cuh:74-78): object o owns faces [begin, next begin). */
typedef struct {
    int32_t begin;
    int32_t mtl;
} tpt_interval;

/* The content of DeviceScene (include/mesh.cuh:80-96).  Every array pointer
 * may be host memory or device memory (detected per pointer, as tpt_render
 * does for its outputs), so the reference's doTrace can pass its
 * thrust::device_vector buffers as they are -- the `trace` kernel's own
 * arguments (path_tracer.cu:297-299): raw_pointer_cast(d_scene.indices.data())
 * etc.  Vec3 arrays are 3 floats per vertex, Mat4 16 floats column-major,
 * Material is tpt_material byte for byte, MtlInterval is tpt_interval.
 * The scene keeps its own copy: the caller's buffers are only read during
 * tpt_scene_create. */
typedef struct {
    const uint32_t* indices;      uint32_t n_faces;      /* 3*n_faces global vertex ids */
    const float* vertices;        const float* normals;  uint32_t n_vertices; /* xyz, object space */
    const tpt_interval* lut;      uint32_t n_objects;
    const float* vert_trans;      const float* normal_trans; /* 16 floats/object, column-major */
    const tpt_material* materials; uint32_t n_materials;   /* empty -> Material() default */
    const tpt_light* lights;      uint32_t n_lights;
    uint32_t flags;               /* TPT_DESC_*; 0 for a zero-initialised desc */
} tpt_scene_desc;

/* desc->lights points at the reference's own DeltaLight array (delta_light.h:
 * 96-130: DeltaLightType, then the PointLight / DirectionalLight / SpotLight
 * union; 52 B, the offsets of tpt_light except that a directional light keeps
 * its direction where tpt_light has pos).  The library repacks it; the
 * union's unused bytes are never read. */
#define TPT_DESC_DELTALIGHT_LAYOUT 0x1

/* Camera (include/camera.h): c2w = m_transform->localToWorld(). */
typedef struct {
    float c2w[16];      /* column-major */
    float vfov;         /* radians */
    float aspect;       /* camera aspect ratio (the reference ignores W/H here) */
    float znear;
} tpt_camera;

typedef struct {
    int32_t width, height;        /* full frame */
    int32_t spp;                  /* samples per pixel (reference: 64 per frame) */
    int32_t max_depth;            /* DEPTH_TRACE (reference: 8), 1..64 */
    uint64_t seed;                /* curand_init seed (reference: time()) */
    /* Interleaved row bands for multi-GPU sharding: this call renders rows y
     * with (y / band_rows) % band_count == band_index.  band_count 1 = all.
     * band_list (below) replaces this deal with an explicit one. */
    int32_t band_rows, band_count, band_index;
    int32_t spp_per_launch;       /* 0 = auto; chunks the spp loop over launches */
    int32_t flags;                /* TPT_FLAG_* */
    int32_t refill;               /* 0 = auto: lanes (of 64) below which a wave stops to shade */
    /* Launch pipeline.  pipe_sets: 0 = auto (3 interleaved band sets
     * from 1024 spp, else 1), 1 = one stream, 2..4 = that many sets (from 256 spp);
     * pipe_chunks: spp chunks per set, 0 = auto (8).  Every schedule is bit-identical
     * to one launch.  The sets run on library-owned streams created at the device's
     * greatest stream priority: HIP gives each priority its own pool of hardware queues
     * (GPU_MAX_HW_QUEUES, 4 by default), and two sets whose streams share a queue run
     * one after the other (-25 % measured).  A host application that issues its own
     * greatest-priority work on the device while tpt_render runs shares those queues. */
    int32_t pipe_sets, pipe_chunks;
    /* Lanes per pixel: 0 = auto (pair mode with delta lights or env IS, else 4 on launches
     * of at most tpt_stats.resident_lanes pixels -- 327,680 on MI355X -- else 1), 1, or
     * 2 = pair mode (scenes with delta lights): a side lane per pixel traces each bounce's
     * shadow rays while the path lane goes on, so a sample's serial chain pays one traversal per bounce; 4 = four
     * lanes run each pixel's path together and split every 4-wide node visit (child k on
     * lane k, leaf children tested at once), a shorter serial chain at a quarter of the
     * pixels per wave (scenes without delta lights, no env IS, ordered traversal; DESIGN.md
     * section 6).  Bit-identical in every mode. */
    int32_t lanes_per_pixel;
    /* 0 = auto: a wave runs its parked triangle tests once this many lanes are blocked on
     * a parked leaf (speculative leaf postponement): 2 in pair mode,
     * else 4.  Bit-identical for any value. */
    int32_t leaf_batch;
    /* TPT_FLAG_WAVEFRONT only: concurrent paths (slots; 0 = every pixel of the call) and the
     * traversing lanes below which a trace wave runs its pass -- finished walks out, the next
     * queued rays in (0 = auto, 40).  Bit-identical for any values. */
    int32_t wf_slots, wf_refill;
    /* Explicit band deal (nullable; a zero-initialised params keeps the interleaved one): this
     * call renders global bands band_list[0 .. band_list_len), band b = rows [b * band_rows,
     * (b + 1) * band_rows) clipped to the frame; distinct ids, a short last band (height not a
     * multiple of band_rows) last; workgroups are dispatched in list order.  band_count and
     * band_index are then ignored.  Any deal is bit-identical to one GPU: the RNG subsequence
     * is the global pixel index (path_tracer.cu:39,320).  Host memory, read during the call. */
    int32_t band_list_len;
    const int32_t* band_list;
    /* Nullable, host memory, ceil(height / band_rows) floats: for each band this call renders,
     * band_cost[b] = the summed life in microseconds of the trace waves that rendered it (megakernel
     * only; 0 under TPT_FLAG_WAVEFRONT); other entries are left as they are.  A deal of the next
     * frame's bands balanced by these costs (tinypathtracer_amd.shard.cost_deal) evens out ranks
     * whose interleaved shares hold the heavy rows. */
    float* band_cost;
} tpt_params;

#define TPT_FLAG_NO_COUNTERS   0x1   /* skip visit counters (traversals still counted) */
#define TPT_FLAG_REF_ORDER     0x2   /* reference right-first traversal, no culling */
#define TPT_FLAG_ENV_IS        0x8   /* opt-in env next-event estimation with importance sampling (A15
                                        re-derived; the reference's trace never calls it, so the image
                                        differs from a reference render) */
#define TPT_FLAG_APPROX_CULL   0x10  /* the ordered traversal's culls without the exactness guards (no
                                        position slack, no sliver re-test, grazing rays culled too;
                                        DESIGN.md section 4): a few
                                        percent faster, and rays whose Moller-Trumbore t is rounding noise
                                        (sliver triangles, grazing edge hits) may then find another hit
                                        than the reference (5 of ~60 G rays over the BASELINE frames) */
#define TPT_FLAG_WAVEFRONT     0x20  /* the wavefront / ray-queue variant (DESIGN.md section 5 "N1"): a logic
                                        kernel and a persistent trace kernel alternate per ray of every
                                        live path, path state in device memory between them; bit-identical
                                        to the megakernel.  lanes_per_pixel, pipe_*, spp_per_launch are
                                        not used */
#define TPT_FLAG_FAST          0x40  /* tolerance mode: the trace kernel built with FMA
                                        contraction, FMA slab tests and the hardware's approximate reciprocal,
                                        sqrt, sin and cos, without the culling guards (implies
                                        TPT_FLAG_APPROX_CULL).  Not bit for bit.  Where the images meet SURVEY
                                        8(d)'s tolerance (mean |d| <= 1e-3, p99 <= 1e-2, >= 99.5 % of pixels
                                        within one 8-bit step): every BASELINE configuration at full
                                        resolution and 1-2 spp, and the full-spp bands of C2 (1024 spp), C3
                                        and C3 + env IS (4096) and C4 (8192).  Where they do not: C5's
                                        full-spp band (2048 spp) meets the mean only -- p99 0.0128 and 96.0 %
                                        within one step (measured with and without the culling guards alike:
                                        the tail is the rounding, not the culls).  Not with
                                        TPT_FLAG_WAVEFRONT */
#define TPT_FLAG_ACCUMULATE    0x4   /* progressive: continue the previous call's per-pixel streams and
                                        sums (same frame size, bands and seed); the output is the mean over
                                        all accumulated samples, bit-identical to one call with their total */

typedef struct {
    uint64_t traversals;          /* traverseBVH calls: primary+extension+probe+shadow */
    uint64_t internal_visits;     /* binary internal nodes popped (reference-order / non-finite rays) */
    uint64_t leaf_tests;          /* leaves popped (triangle tests) */
    uint64_t shade_hits;          /* extension-ray hits shaded */
    uint64_t pixels;              /* pixels rendered by this call */
    uint64_t samples;             /* pixels * spp */
    double rng_init_ms;           /* setupRandSeed equivalent */
    double trace_ms;              /* trace phase, first launch start to last launch end (HIP events) */
    double resolve_ms;            /* copyToFB equivalent */
    double total_ms;              /* whole tpt_render, host wall */
    int32_t trace_launches;
    int32_t wg_waves;             /* waves per trace workgroup the launches ran (1, 2 or 4: the build's shape
                                     for the variant family; 0 with TPT_FLAG_WAVEFRONT) */
    uint64_t wide_visits;         /* 4-wide internal nodes popped (ordered traversal) */
    uint64_t accumulated_spp;     /* samples per pixel in the output (> spp with TPT_FLAG_ACCUMULATE) */
    double trace_kernel_ms;       /* sum of the trace launches' own durations (HIP events per launch);
                                     > trace_ms when the launch pipeline overlaps them */
    uint64_t local_rays;          /* of `traversals`, the direct probes resolved in the shading pass without
                                     a BVH traversal (no emissive triangle, or a miss of the <= 4-emitter
                                     inline test); traversals - local_rays = BVH traversals run */
    double tree_wait_ms;          /* host wall time this call waited for a tpt_scene_build_async's host
                                     traversal-tree build, after enqueueing the RNG initialisation */
    uint64_t resident_lanes;      /* the device's resident trace lanes (hipDeviceProp_t CUs x 4 SIMDs x
                                     the one-lane variant's waves per SIMD x 64; MI355X 327,680): launches of
                                     at most this many pixels run four lanes per pixel (lanes_per_pixel 0),
                                     below twice it the latency-oriented (drained) variants */
    int32_t lanes_per_pixel;      /* the lane mode the trace launches ran: 1, 2 (pair) or 4 */
    int32_t drained;              /* 1: the drained-launch rule applied (refill, leaf batch, DRAIN variants) */
} tpt_stats;

typedef struct tpt_scene tpt_scene;
typedef struct tpt_env tpt_env;

/* Library identity and errors. */
const char* tpt_version(void);
const char* tpt_last_error(void);
int tpt_device_count(void);

/* Upload a scene to `device` (hipSetDevice index).  Replaces
 * Scene::copySceneToDevice (mesh.cu:309-397). */
tpt_status tpt_scene_create(const tpt_scene_desc* desc, int device, tpt_scene** out);
/* World transform + LBVH build on the device (path_tracer.cu:536-542,
 * bvh.cu:304-331) and the packed traversal layout. */
tpt_status tpt_scene_build(tpt_scene* scene);
/* tpt_scene_build whose host half -- the SAH traversal trees over the LBVH's
 * leaf boxes -- continues on a host thread after the call returns (the device
 * LBVH build and its read-back are done).  The next call that traces the scene
 * waits for it: tpt_render / tpt_render_frames after enqueueing the per-pixel
 * RNG initialisation (setupRandSeed, path_tracer.cu:513), so the two overlap;
 * tpt_debug_trace_rays first.  A failure of the host half is reported by that
 * call.  tpt_scene_build / _async and tpt_scene_destroy supersede a pending
 * one.  The scene is the same as tpt_scene_build's. */
tpt_status tpt_scene_build_async(tpt_scene* scene);
/* Host threads of the traversal-tree build inside tpt_scene_build (the SAH
 * 4-wide tree): < 0 = auto (the cores this process may
 * use: its affinity mask capped by the cgroup CPU quota), 0 or 1 = serial.
 * Every setting builds the same tree.  Processes sharing a host (one per GPU)
 * pass their share of the cores. */
tpt_status tpt_scene_set_build_threads(tpt_scene* scene, int32_t threads);
/* New local-to-world matrices for objects [first_object, first_object + n_objects): each
 * 16 floats, column-major, host memory, as tpt_scene_desc's.  normal_trans: nullable; null:
 * computed from vert_trans as the glTF loader computes it (the inverse transpose of the
 * linear part).  The vertices stay on the device; the matrices are uploaded on the scene's
 * stream, a pending tpt_scene_build_async is joined and superseded, and the scene is
 * unbuilt afterwards: call tpt_scene_build, tpt_scene_build_async or tpt_scene_refit before
 * the next render.  The rebuilt scene is the scene tpt_scene_create + tpt_scene_build make of a
 * desc with these matrices, bit for bit (world vertices, BVH, rendered frames).  A
 * progressive accumulation (TPT_FLAG_ACCUMULATE) does not survive it: its sums belong to
 * the scene as it was, so render the next frame without the flag.
 * TPT_ERR_INVALID_ARG (nothing changes): null scene or vert_trans, n_objects == 0, a
 * range past the scene's object count. */
tpt_status tpt_scene_set_transforms(tpt_scene* scene, uint32_t first_object, uint32_t n_objects,
                                    const float* vert_trans, const float* normal_trans);
/* New object-space positions for the global vertex ids [first_vertex, first_vertex +
 * n_vertices): xyz, 3 floats each, as tpt_scene_desc's vertices.  normals: nullable; null:
 * the stored normals stay as they are.  Each pointer may be host or device memory (of the
 * scene's device), detected per pointer as tpt_scene_create does.  Topology (indices, lut),
 * materials and matrices are untouched.  A pending tpt_scene_build_async is joined and
 * superseded, and the scene is unbuilt afterwards: call tpt_scene_build,
 * tpt_scene_build_async or tpt_scene_refit before the next render.  The rebuilt scene is the scene
 * tpt_scene_create + tpt_scene_build make of a desc holding these vertices, bit for bit
 * (tpt_scene_read_world, tpt_scene_read_bvh, rendered frames).  A progressive accumulation
 * does not survive it, as for tpt_scene_set_transforms.  tpt_scene_build is a full rebuild;
 * tpt_scene_refit (below) keeps the trees' topology and recomputes their boxes on the device
 * (DESIGN.md section 5 "Deforming meshes", "BVH refit").
 * TPT_ERR_INVALID_ARG (nothing changes): null scene or vertices, n_vertices == 0, a range
 * past the scene's vertex count, a device buffer of another device. */
tpt_status tpt_scene_set_vertices(tpt_scene* scene, uint32_t first_vertex, uint32_t n_vertices,
                                  const float* vertices, const float* normals);
/* What a tpt_scene_refit did, and the number a caller decides a rebuild by. */
typedef struct tpt_refit_stats {
    int32_t rebuilt;      /* 1: the call fell back to a full tpt_scene_build */
    int32_t launches;     /* kernels the call launched (a fallback's build kernels are not counted) */
    int32_t slivers;      /* sliver triangles found (trace.hip "Culling") */
    float cull_eps;       /* the recomputed cull slack */
    double ms;            /* device time of the call, by events on the scene's stream */
    double cost;          /* the main 4-wide tree now: the summed surface areas of all child boxes of all
                           * its nodes over the surface area of the union of the root's child boxes
                           * (areas and sum in double, a fixed order: the same value every run) */
    double cost_built;    /* the same quantity as the last full build left it */
} tpt_refit_stats;
/* In place of tpt_scene_build after tpt_scene_set_vertices and / or tpt_scene_set_transforms:
 * leaves the scene built, with no host tree work.  Kept from the last full build: the triangle
 * order (the sorted Morton keys tpt_scene_read_bvh returns are then stale), the LBVH topology,
 * the topology, links and emitter bits of both 4-wide SAH trees, the stack depth.  Recomputed
 * on the device, on the scene's stream: the world vertices and normals (bit for bit a
 * rebuild's), the leaf boxes, the triangle and shading records, every LBVH node box, every
 * child box of every 4-wide node (a leaf child: the exact leaf box; an inner child: the exact
 * min/max union of that node's child boxes), one kernel launch per tree level, deepest
 * first.  Recomputed on the host from small read-backs: the boxes' finiteness, the cull slack,
 * the sliver list (only when there are slivers do the leaf boxes come back), the emitter
 * boxes.  A progressive accumulation does not survive it.
 * A full tpt_scene_build runs inside the call (stats->rebuilt = 1) when the scene holds no
 * complete build (never built, or an asynchronous build superseded by a tpt_scene_set_*
 * before its trees were uploaded), when it was built without the SAH tree (one triangle, or
 * non-finite boxes), or when the refit meets a non-finite world vertex or box.  A pending
 * asynchronous build that was not superseded is finished first.
 * Against a rebuild: where two different triangles are hit at a bit-equal closest t, the
 * kernel's tie rule picks the larger sorted position, and after a refit the positions are
 * those of the last full build, so such a ray may return the other triangle.  Every other
 * ray returns the same hit bit for bit (the hit depends only on the leaves' exact boxes and
 * positions, wide_bvh.cpp).  The trees' quality degrades as the deformation grows: the
 * library takes no decision from stats->cost / cost_built, the caller does (DESIGN.md
 * section 5 "BVH refit" has a rule of thumb).  Not provided: partial (dirty-subtree) refits,
 * topology changes, re-sorting.
 * stats: nullable.  TPT_ERR_INVALID_ARG: null scene. */
tpt_status tpt_scene_refit(tpt_scene* scene, tpt_refit_stats* stats);
void tpt_scene_destroy(tpt_scene* scene);

/* Equirect environment, RGBA8, row 0 = bottom (FreeImage order), already in
 * RGB channel order (texture.cu:33-47 swizzle applied by the caller). */
tpt_status tpt_env_create(const uint8_t* rgba, int32_t width, int32_t height, int device, tpt_env** out);
void tpt_env_destroy(tpt_env* env);

/* Env map from an image file: EnvLight(file) (include/env_light.cuh:8-18,
 * src/texture.cu:64-171, include/picture.h:19-45).  Decodes JPEG (baseline and
 * progressive Huffman, libjpeg's default islow IDCT / fancy upsampling / YCbCr
 * tables) or binary PPM natively into the texel layout tpt_env_create takes
 * (RGBA8, row 0 = bottom).  Errors: TPT_ERR_IO (cannot open), TPT_ERR_PARSE
 * (unsupported or corrupt image, e.g. grayscale, which the reference's
 * Texture also rejects). */
tpt_status tpt_env_load(const char* path, int device, tpt_env** out);
/* The decoder alone: *rgba is allocated by the library (free with
 * tpt_image_free), width*height*4 bytes, row 0 = bottom. */
tpt_status tpt_image_load(const char* path, uint8_t** rgba, int32_t* width, int32_t* height);
void tpt_image_free(uint8_t* rgba);
/* One frame == doTrace: setupRandSeed, trace (spp), copyToFB.
 *   radiance_out: nullable, width*height*3 floats = color/spp, row 0 = bottom;
 *                 host or device pointer (detected).  Only band rows written.
 *   bgra_out:     nullable, width*height*4 bytes, row 0 = top, B,G,R written,
 *                 alpha untouched (copyToFB, path_tracer.cu:451-471).
 *   env:          nullable -> black on miss.
 * Device outputs are written on the library's own stream and are complete when
 * tpt_render returns; no other stream may have work pending that reads or
 * writes them when the call starts (the caller synchronises its stream first;
 * the Python host does this for torch tensors). */
tpt_status tpt_render(tpt_scene* scene, const tpt_env* env, const tpt_camera* camera,
                      const tpt_params* params, float* radiance_out, uint8_t* bgra_out,
                      tpt_stats* stats);

/* A batch of independent frames in one trace launch: frame f is a doTrace
 * with seed seeds[f] (the reference re-seeds every frame from time(),
 * path_tracer.cu:493-494,513); all frames share params (size, spp, bands,
 * flags) and params->seed is ignored.  Frame f is bit-identical to
 * tpt_render with seed seeds[f].  Used to keep every GPU of a node busy on
 * its share of several frames at once (bench.py weak scaling).
 *   radiance_outs / bgra_outs: nullable arrays of n_frames nullable pointers,
 *   each as in tpt_render.  stats: summed over the batch. */
tpt_status tpt_render_frames(tpt_scene* scene, const tpt_env* env, const tpt_camera* camera,
                             const tpt_params* params, int32_t n_frames, const uint64_t* seeds,
                             float* const* radiance_outs, uint8_t* const* bgra_outs, tpt_stats* stats);

/* Adaptive sampling (DESIGN.md section 5 "Adaptive sampling"): every 16x16-pixel tile of the
 * frame is rendered until its error estimate falls below `target`, at most to max_spp.
 *
 * Schedule: every tile gets min_spp samples in two halves; then, with n = min_spp, each tile's
 * error E is estimated from its pixels' n-spp radiance I and n/2-spp radiance A (Dammertz et
 * al. 2010, the first half of the samples as the half buffer):
 *   e = (|I.r - A.r| + |I.g - A.g| + |I.b - A.b|) / sqrt(max(I.r + I.g + I.b, 1e-4)),
 *   E = the mean of e over the tile's in-frame pixels (float32, a fixed summation order).
 * A tile with E < target stops with n samples; the others get n more, n doubles and the
 * estimate repeats, until n == max_spp.  A tile still at or above the target there counts in
 * unconverged_tiles.  A tile with a non-finite pixel has E = NaN, which is below no target: it
 * runs to max_spp and counts as unconverged.  target 0 renders every tile to max_spp, +inf
 * every tile to min_spp.
 *
 * So every tile holds min_spp * 2^i samples, and every pixel of radiance_out and bgra_out
 * equals tpt_render's at its tile's count, bit for bit, with the same seed, max_depth and
 * flags: the tiles continue the per-pixel streams and sums a progressive render would.
 *
 *   params:        width, height, max_depth, seed, flags, lanes_per_pixel, refill, leaf_batch
 *                  as in tpt_render (each pass picks its lane mode by its own tile count);
 *                  spp, spp_per_launch and the pipe_* fields are ignored.
 *   radiance_out, bgra_out: as tpt_render's; at least one is non-null.
 *   tile_spp_out:   nullable, ceil(height / 16) * ceil(width / 16) entries, row 0 = bottom:
 *                   the samples each tile holds.  Host or device memory, like the images.
 *   tile_error_out: nullable, as many floats: each tile's last estimate.
 *
 * TPT_ERR_INVALID_ARG, nothing written: min_spp odd or < 2; max_spp not min_spp * 2^j; a NaN
 * or negative target; unknown adaptive flags (none are defined); TPT_FLAG_WAVEFRONT or
 * TPT_FLAG_ACCUMULATE; band_count > 1, a band_index, a band_list or a band_cost (the whole
 * frame only); both image outputs null; a frame wider or higher than 1,048,576 pixels; and
 * whatever tpt_render refuses.  The scene's progressive state is invalid afterwards: a later
 * TPT_FLAG_ACCUMULATE render starts over.  The snapshot of the sums (12 bytes per pixel) stays
 * with the scene. */
typedef struct {
    int32_t min_spp, max_spp;     /* even, >= 2; min_spp * 2^j */
    float target;                 /* >= 0, +inf allowed */
    int32_t flags;                /* 0 */
} tpt_adaptive_params;

typedef struct {
    uint64_t samples;             /* sum over the tiles of in-frame pixels * samples */
    uint64_t pixels;              /* width * height */
    uint64_t traversals;          /* as tpt_stats */
    int32_t passes;               /* trace passes: the two halves of min_spp, then one per doubling */
    int32_t unconverged_tiles;    /* tiles at or above the target (or NaN) at max_spp */
    double trace_ms;              /* the passes' trace launches (HIP events), summed */
    double error_ms;              /* the snapshot and estimate kernels, summed */
    double total_ms;              /* whole call, host wall */
} tpt_adaptive_stats;

tpt_status tpt_render_adaptive(tpt_scene* scene, const tpt_env* env, const tpt_camera* camera,
                               const tpt_params* params, const tpt_adaptive_params* adaptive,
                               float* radiance_out, uint8_t* bgra_out, int32_t* tile_spp_out,
                               float* tile_error_out, tpt_adaptive_stats* stats);

/* ---- after the render: first-hit feature buffers and the denoiser (DESIGN.md section 5 "Post-pass") ---- */

/* First-hit feature buffers (AOVs).  Each pointer is nullable and may be host
 * or device memory (detected per pointer, as tpt_render does for its outputs);
 * device outputs follow tpt_render's stream rule. */
typedef struct {
    float*   albedo;    /* W*H*3: the hit material's base colour; (1, 1, 1) on a miss */
    float*   normal;    /* W*H*3: the shading normal of the hit prelude; (0, 0, 0) on a miss */
    float*   depth;     /* W*H:   hitDist along the unit ray; 0 on a miss */
    int32_t* face;      /* W*H:   face id; -1 on a miss */
    int32_t* material;  /* W*H:   material id; -1 on a miss */
} tpt_aov;              /* all row 0 = bottom, like radiance_out */

/* One deterministic ray per pixel through the pixel centre (sampleRays,
 * path_tracer.cu:42-59, with the jitter fixed at (0.5, 0.5); no RNG is consumed)
 * through the render's own closest-hit traversal, then the hit prelude of
 * path_tracer.cu:364-374: the buffers describe the surface the render's primary
 * ray finds.  Whole frame only (bands and deals do not apply; in a multi-GPU run
 * rank 0 calls it for the gathered frame).  A pending tpt_scene_build_async is
 * waited for first.  trace_ms: nullable, the kernel's duration (HIP events).
 * TPT_ERR_INVALID_ARG: unbuilt scene, width or height <= 0, null camera or out,
 * or every pointer of out null. */
tpt_status tpt_render_aov(tpt_scene* scene, const tpt_camera* camera, int32_t width, int32_t height,
                          const tpt_aov* out, double* trace_ms);

/* Mirror-path feature buffers: tpt_render_aov continued through perfect mirrors
 * (DESIGN.md section 5 "Post-pass" holds the definition).  A hit is a mirror when its
 * material has !(eta > 0), metallic > 0 and !(emission_factor > 0): getNewDirection's
 * branch order, and an emitter ends a path.  The reference's metal reflects without a random
 * number, so the path is followed exactly: from the hit point along reflect(d, n) about the
 * shading normal, traced as the render traces an extension ray from that face, up to
 * max_bounces mirrors.  The buffers describe the first surface that is no mirror (glass is
 * one such: its two lobes are a coin flip), or the mirror met at the cap:
 *   face, material, normal: that surface's; -1, -1, 0 when the path leaves the scene;
 *   albedo: the product of the base colours of every surface met, mirrors included, so that
 *     demodulation divides a reflection by the tint it carries; on a miss the mirrors' alone;
 *   depth: the distance travelled along the whole path, on a miss up to the last mirror;
 *   bounces_out: nullable, W*H (host or device memory as out's pointers): mirrors followed.
 * With max_bounces 0, and in a scene without a mirror, every buffer equals tpt_render_aov's
 * bit for bit.  Deterministic; no RNG is consumed.  tpt_denoise and tpt_denoise_svgf take
 * the result as `guides` unchanged.  tpt_temporal and tpt_temporal_motion do not: they
 * reproject the first hit and compare its material, so they stay on tpt_render_aov's buffers
 * (tpt_temporal_path is the pass for these).
 * stats: nullable.
 * TPT_ERR_INVALID_ARG: tpt_render_aov's refusals (out itself may be null when bounces_out is
 * not: at least one output is needed), null params, max_bounces outside 0..64, flags != 0. */
typedef struct {
    int32_t max_bounces;     /* 0..64, as tpt_params.max_depth's range */
    int32_t flags;           /* 0; unknown bits are refused */
} tpt_aov_path_params;

typedef struct {
    double   trace_ms;       /* the kernel's duration (HIP events) */
    uint64_t followed;       /* pixels that followed at least one mirror */
    int32_t  deepest;        /* the largest bounce count of the frame */
} tpt_aov_path_stats;

tpt_status tpt_render_aov_path(tpt_scene* scene, const tpt_camera* camera, int32_t width, int32_t height,
                               const tpt_aov_path_params* params, const tpt_aov* out, int32_t* bounces_out,
                               tpt_aov_path_stats* stats);

/* tpt_render_aov_path with where each path ended as a seventh output, for tpt_temporal_path:
 *   points_out: W*H*3 floats (host or device memory as the others).  Where the path ends on a
 *     surface (material >= 0): the world point origin_k + t d_k of that hit in float32, formed
 *     as the walk advances an origin from mirror to mirror.  Where it leaves the scene
 *     (material -1): the unit direction d_k of its last ray; with no mirror followed that is
 *     the pixel-centre direction.
 * Every other output is tpt_render_aov_path's bit for bit, and with points_out null the call is
 * tpt_render_aov_path.  The refusals are tpt_render_aov_path's (points_out counts as an
 * output). */
tpt_status tpt_render_aov_path_points(tpt_scene* scene, const tpt_camera* camera, int32_t width, int32_t height,
                                      const tpt_aov_path_params* params, const tpt_aov* out, int32_t* bounces_out,
                                      float* points_out, tpt_aov_path_stats* stats);

#define TPT_DENOISE_DEMODULATE 0x1  /* filter radiance / max(albedo, 1e-3), multiply back afterwards */
#define TPT_DENOISE_DIRECT     0x2   /* A/B: steps 1 and 2 through the direct kernel too instead of the
                                        LDS-staged one (bit-identical output) */

typedef struct {
    int32_t iterations;      /* 0..8; 0 = copy */
    float   sigma_color;     /* > 0 */
    float   sigma_normal;    /* > 0 */
    float   sigma_depth;     /* > 0, relative */
    int32_t flags;           /* TPT_DENOISE_* */
} tpt_denoise_params;

typedef struct { double pack_ms, filter_ms, resolve_ms; } tpt_denoise_stats;

/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) of a radiance frame,
 * guided by its first-hit albedo, normal and depth (guides->face / material are
 * ignored; the three others are required).  The filter is defined in DESIGN.md
 * section 5 "Post-pass": iteration i has step 2^i and the 5x5 B3-spline taps h = [1/16, 1/4,
 * 3/8, 1/4, 1/16] (taps outside the frame skipped), each weighted by
 * exp(-|dc|^2 / (sigma_color 2^-i)^2) exp(-|dn|^2 / sigma_normal^2)
 * exp(-dz^2 / (sigma_depth^2 max(z(p)^2, 1e-12))).  iterations 0: the output is the
 * input bit for bit.  Non-finite input radiance is the caller's problem: a NaN or
 * infinite pixel spreads to every pixel whose taps reach it.
 *   radiance_in / radiance_out: W*H*3 floats, row 0 = bottom; may be the same
 *     pointer; radiance_out nullable.
 *   bgra_out: nullable, as tpt_render's (row 0 = top, B,G,R written, alpha
 *     untouched, truncating toUChar).
 * Inputs and outputs may be host or device memory (tpt_render's stream rule for
 * device memory); all work is complete when the call returns.  `scene` supplies the
 * device, the stream and the scratch planes, which stay with it between calls
 * (48 B per pixel, and up to 44 B more to stage host buffers); it need not be
 * built.  Deterministic (no atomics).
 * TPT_ERR_INVALID_ARG: null scene / radiance_in / guides / params, a missing
 * albedo, normal or depth guide, width or height <= 0, iterations outside 0..8,
 * a sigma that is not > 0, both outputs null. */
tpt_status tpt_denoise(tpt_scene* scene, int32_t width, int32_t height, const float* radiance_in,
                       const tpt_aov* guides, const tpt_denoise_params* params, float* radiance_out,
                       uint8_t* bgra_out, tpt_denoise_stats* stats);

/* Temporal reprojection and accumulation across frames (DESIGN.md section 5 "Post-pass").
 * A history belongs to one frame size and to the scene it was created from, which
 * supplies the device and the stream and need not be built; destroy the history
 * before its scene.  It holds two sets of three float4 planes (accumulated colour +
 * history length; normal + depth; luminance moments + material id), 96 B per pixel,
 * and up to 56 B per pixel more to stage host buffers (tpt_temporal_motion: 68 B), 4 B
 * per face and 96 B per object (tpt_temporal_deform: 24 B per vertex more).  After tpt_history_create and after tpt_history_reset
 * there is no state: the next tpt_temporal starts over. */
typedef struct tpt_history tpt_history;
tpt_status tpt_history_create(tpt_scene* scene, int32_t width, int32_t height, tpt_history** out);
tpt_status tpt_history_reset(tpt_history* h);
void tpt_history_destroy(tpt_history* h);

/* History clipping (DESIGN.md section 5 "History clipping" holds the definition): a setting of
 * the history that every temporal entry point obeys, off by default.  The reprojection rules
 * test geometry only, so what changes because something else moved -- a moved object's shadow,
 * its reflection on a wall that stood still -- is reprojected as if nothing had happened.  With
 * the clip on, each call first takes, per pixel and channel, the mean mu and the standard
 * deviation sigma of the colour it accumulates over the pixels of a (2 radius + 1)^2 window that
 * are similar to the centre (the same material -- and bounce count in tpt_temporal_path -- and on
 * a hit a depth within the call's depth_tol of the centre's and a normal with n(q) . n(p) >=
 * normal_min), and a reprojected pixel's gathered history colour is clamped to [mu - gamma
 * sigma, mu + gamma sigma] before it is blended.  A history that the clamp moved has its length
 * capped at max_history (before the + 1) and its luminance moments shifted to the clamped colour
 * at their variance.  A window with fewer than four similar pixels gives no box.  The setting
 * survives tpt_history_reset.  The box's two float4 planes, 32 B per pixel, are allocated at the
 * first clipped call.  With the clip off every entry point launches exactly the kernels it
 * launches without this feature.
 * TPT_ERR_INVALID_ARG (nothing is changed): a null history, radius outside 1..3, gamma NaN,
 * infinite or not > 0, max_history outside 1..65536, an unknown flag; a null out. */
typedef struct {
    int32_t radius;        /* 1..3: the window is (2 radius + 1)^2 pixels */
    float   gamma;         /* finite, > 0: half-width of the box in standard deviations */
    int32_t max_history;   /* 1..65536: a clipped pixel's history length is capped at this before the +1 */
    int32_t flags;         /* 0; unknown bits are refused */
} tpt_clip_params;
typedef struct {
    double   box_ms;       /* the box kernel's duration (HIP events); 0 when clipping is off */
    uint64_t boxed;        /* pixels of the last call whose window gave a box (n >= 4) */
    uint64_t clipped;      /* reprojected pixels of the last call whose history was moved by the clip */
} tpt_clip_stats;
tpt_status tpt_history_set_clip(tpt_history* h, const tpt_clip_params* p);   /* p null: off (the default) */
tpt_status tpt_history_clip_stats(const tpt_history* h, tpt_clip_stats* out); /* of the last temporal call */

#define TPT_TEMPORAL_DEMODULATE 0x1   /* accumulate radiance / max(albedo, 1e-3); multiply the current albedo back */
#define TPT_TEMPORAL_TILES      0x2   /* A/B: lanes in 16x16 tiles instead of 64-pixel row segments
                                         (bit-identical output) */

typedef struct {
    float   alpha;         /* (0, 1]: least weight of the new frame */
    float   depth_tol;     /* > 0, relative */
    float   normal_min;    /* [-1, 1]: least n'(q) . n(p) */
    int32_t max_history;   /* 1..65536 */
    int32_t flags;         /* TPT_TEMPORAL_* */
} tpt_temporal_params;

typedef struct {
    double   kernel_ms;    /* the kernel's duration (HIP events) */
    uint64_t reprojected;  /* pixels that found history */
} tpt_temporal_stats;

/* One frame through the history.  Each pixel's first hit (a miss: its direction, a
 * point at infinity) is projected into the previous call's camera; the four bilinear
 * taps there are kept where the previous frame saw the same material and, on a hit,
 * a depth within depth_tol (relative) of the distance to the previous origin and a
 * normal with n' . n >= normal_min.  With valid weights summing to at least 1/16 the
 * pixel is reprojected: N = min(N' + 1, max_history), a = max(alpha, 1 / N), and the
 * colour and the luminance moments move a of the way from the weighted history to
 * this frame.  Otherwise it is disoccluded: N = 1 and the output is the input bit
 * for bit.  The new state and `camera` then replace the old.  Only the camera may
 * move between frames, not the scene (tpt_temporal_motion follows objects that moved).
 *   guides: normal, depth and material (tpt_render_aov) are required, albedo only with
 *     TPT_TEMPORAL_DEMODULATE; face is ignored.
 *   radiance_in / radiance_out: W*H*3 floats, row 0 = bottom; may be the same pointer.
 *   variance_out: nullable, W*H: max(M2 - M1^2, 0) of the accumulated luminance
 *     (of the demodulated colour under TPT_TEMPORAL_DEMODULATE).
 *   history_len_out: nullable, W*H: N.
 *   bgra_out: nullable, as tpt_denoise's.  At least one of radiance_out and bgra_out.
 * Inputs and outputs may be host or device memory (tpt_render's stream rule for
 * device memory); all work is complete when the call returns.  Deterministic: no
 * floating-point atomics.  Non-finite input radiance is the caller's problem: it
 * stays in the history until the pixel is disoccluded or the history is reset.
 * TPT_ERR_INVALID_ARG (nothing is written and the history is left as it was): null
 * h / camera / radiance_in / guides / params, a missing required guide, alpha outside
 * (0, 1], depth_tol not > 0, normal_min outside [-1, 1], max_history outside
 * 1..65536, an unknown flag, radiance_out and bgra_out both null. */
tpt_status tpt_temporal(tpt_history* h, const tpt_camera* camera, const float* radiance_in,
                        const tpt_aov* guides, const tpt_temporal_params* params,
                        float* radiance_out, float* variance_out, float* history_len_out,
                        uint8_t* bgra_out, tpt_temporal_stats* stats);

/* tpt_temporal for a scene whose objects moved (tpt_scene_set_transforms) since the
 * previous call on this history, by either entry point: both record the transforms of the
 * scene the history was created from.  The caller has rebuilt that scene and rendered
 * `guides` from it.  A hit pixel's face id names its object; with M' the object's previous
 * matrix and M its current one (tpt_motion_matrices), the first hit X is taken to
 * X' = M' M^-1 X, where that point of the object was in the previous frame, and X' is what is
 * projected into the previous camera and measured against the previous origin; the normal
 * test compares the previous frame's normals with normalize((M' M^-1)_lin^-T n).  An object
 * whose matrices are bit-equal takes tpt_temporal's path bit for bit: with nothing moved the
 * outputs and the new state are tpt_temporal's.  A hit pixel is disoccluded when its face id
 * is outside [0, n_faces) or its object is untracked (tpt_motion_matrices).  Misses reproject
 * their direction as before.  DESIGN.md section 5 "Moving objects" holds the definition.
 *   guides: as tpt_temporal's, and face is required.
 *   motion_out: nullable, W*H*2: the reprojected (after the snap) minus the pixel's own
 *     coordinates, (fx - x, fy - y) in pixels, wherever the reprojection lies in front of the
 *     previous camera and is finite -- whether or not its taps were accepted, inside the frame
 *     or not; (0, 0) elsewhere, for untracked pixels and when there is no previous state.
 * Everything else is tpt_temporal's, the refusals too (and a missing face guide).
 * Not tracked: shading that changes because something else moved -- a moved object's shadow
 * or its reflection on a wall that stood still is reprojected as if nothing had happened,
 * and `alpha` is what bounds that lag (tpt_history_set_clip shortens it).  Lights do not move;
 * meshes that deform are tpt_temporal_deform's. */
tpt_status tpt_temporal_motion(tpt_history* h, const tpt_camera* camera, const float* radiance_in,
                               const tpt_aov* guides, const tpt_temporal_params* params,
                               float* radiance_out, float* variance_out, float* history_len_out,
                               float* motion_out, uint8_t* bgra_out, tpt_temporal_stats* stats);

/* tpt_temporal for a scene whose vertices moved (tpt_scene_set_vertices; or whose objects
 * moved, tpt_scene_set_transforms: the world vertices hold the matrices) since the previous
 * tpt_temporal_deform call on this history.  The caller has rebuilt the scene the history was
 * created from and rendered `guides` (tpt_render_aov's first-hit buffers, not the mirror-path
 * ones) from it.  Unlike the other temporal entry points this one reads the scene's world
 * buffers: an unbuilt scene is refused, a pending tpt_scene_build_async is waited for.
 * The history keeps a snapshot of the scene's world vertices and normals (24 B per vertex,
 * allocated at the first call), copied device to device on the scene's stream at the end of
 * every call.  It is the previous frame's only if no other call on this history -- another
 * temporal entry point, or tpt_history_reset -- came in between; otherwise, with a valid
 * history, every hit pixel is disoccluded for that one frame and misses reproject as ever.
 * A hit pixel's face id f names its triangle, indices[3f..3f+2].  If the triangle's 9 world
 * position floats and 9 world normal floats are bit-equal to the snapshot's, the pixel takes
 * tpt_temporal's path untouched: with nothing deformed the outputs and the new state are
 * tpt_temporal's bit for bit.  Otherwise (u, v) are the barycentrics of the pixel-centre ray on
 * the current triangle, w = 1 - u - v, and with a', b', c', na', nb', nc' the snapshot's corners
 *   X' = (w a' + u b') + v c',   ne = normalize((w na' + u nb') + v nc'):
 * X' is projected into the previous camera and measured against the previous origin, and the
 * normal test compares the previous frame's normals with ne.  A hit pixel is disoccluded when
 * its face id is outside [0, n_faces), its triangle is flat (determinant 0) or u, v or X' is
 * not finite.  guides, motion_out and everything else are tpt_temporal_motion's, the refusals
 * too (and an unbuilt scene).  DESIGN.md section 5 "Deforming meshes" holds the definition.
 * Not tracked: a deforming object's shadow and its reflections (in mirrors too), reprojected as
 * if nothing had happened (tpt_history_set_clip shortens that lag); topology changes.  Lights do
 * not move. */
tpt_status tpt_temporal_deform(tpt_history* h, const tpt_camera* camera, const float* radiance_in,
                               const tpt_aov* guides, const tpt_temporal_params* params,
                               float* radiance_out, float* variance_out, float* history_len_out,
                               float* motion_out, uint8_t* bgra_out, tpt_temporal_stats* stats);

/* tpt_temporal on mirror-path guides: accumulation that follows reflections in perfect mirrors
 * under a moving camera (DESIGN.md section 5 "Temporal accumulation through mirrors" holds the
 * definition).  tpt_temporal reprojects the first hit, so on a mirror it blends in the history
 * of whatever the mirror showed from the previous camera.  Here each pixel carries its path:
 *   path_guides: tpt_render_aov_path's normal, depth D (the whole path's length) and material,
 *     all required; albedo (the path's product) only with TPT_TEMPORAL_DEMODULATE;
 *   bounces: W*H, the mirrors followed k; points: W*H*3, tpt_render_aov_path_points' output P.
 *     Both required, host or device memory as the others.
 * A pixel with k = 0 takes tpt_temporal's rules, and its taps must have stored k' = 0 too.  A
 * pixel with k > 0 that ends on a surface reprojects X = o + D d, the virtual image of its
 * terminal point (a fixed world point for chains of planar mirrors); a tap is valid when
 * k' = k, the terminal material is equal, n' . n >= normal_min, |D' - |X - o'|| <= depth_tol
 * |X - o'|, and |P' - P| <= point_tol D sensor_h / height of this camera: the terminal world
 * points lie within point_tol pixel footprints of each other.  A pixel with k > 0 whose path
 * left the scene reprojects its direction as a miss does; a tap is valid when k' = k, m' = -1
 * and |d' - d| <= point_tol sensor_h / height.  Everything else -- the taps, the 1/16 rule, the
 * accumulation, demodulation, disocclusion, the outputs -- is tpt_temporal's.  On a curved
 * mirror, or one with tilted shading normals, the point rule rejects what the virtual image
 * gets wrong: such pixels mostly disocclude (tpt_denoise_svgf's short-history estimate is for
 * those) instead of ghosting.
 * The history keeps k in a word of its third plane that was unused and P in a fourth plane per
 * set, allocated at the first tpt_temporal_path call: 32 B per pixel more, and up to 16 B more
 * to stage host buffers.  In a scene without a mirror, or with max_bounces 0 buffers, the
 * outputs and the state are tpt_temporal's bit for bit.  The entry points may alternate on one
 * history: after a tpt_temporal or tpt_temporal_motion call every stored k' is 0, so the next
 * tpt_temporal_path call disoccludes its k > 0 pixels.  Moving objects are not followed: after
 * tpt_scene_set_transforms reset the history, or use tpt_temporal_motion on first-hit guides.
 * TPT_ERR_INVALID_ARG (nothing is written and the history is left as it was): tpt_temporal's
 * refusals, null bounces or points, point_tol not > 0. */
typedef struct {
    float   alpha;         /* as tpt_temporal_params */
    float   depth_tol;
    float   normal_min;
    int32_t max_history;
    int32_t flags;         /* TPT_TEMPORAL_* */
    float   point_tol;     /* > 0, in pixel footprints */
} tpt_temporal_path_params;

tpt_status tpt_temporal_path(tpt_history* h, const tpt_camera* camera, const float* radiance_in,
                             const tpt_aov* path_guides, const int32_t* bounces, const float* points,
                             const tpt_temporal_path_params* params, float* radiance_out,
                             float* variance_out, float* history_len_out, uint8_t* bgra_out,
                             tpt_temporal_stats* stats);

#define TPT_SVGF_DEMODULATE 0x1   /* filter radiance / max(albedo, 1e-3), multiply back afterwards */
#define TPT_SVGF_DIRECT     0x2   /* A/B: steps 1 and 2 through the direct kernel too instead of the
                                     LDS-staged one (bit-identical output) */

typedef struct {
    int32_t iterations;    /* 0..8 */
    float   sigma_lum;     /* > 0, in standard deviations of the luminance */
    float   sigma_normal;  /* > 0 */
    float   sigma_depth;   /* > 0, relative */
    int32_t min_history;   /* 1..65536: a history shorter than this takes the spatial variance estimate */
    int32_t flags;         /* TPT_SVGF_* */
} tpt_svgf_params;

typedef struct {
    double   pack_ms, estimate_ms, filter_ms, resolve_ms;   /* the kernels' durations (HIP events) */
    uint64_t estimated;                                      /* pixels that took the spatial estimate */
} tpt_svgf_stats;

/* Variance-guided a-trous filter (Schied et al. 2017, SVGF) of a radiance frame,
 * guided by its first-hit normal and depth and by the per-pixel variance of its
 * luminance, which is filtered alongside the colour.  The filter is defined in
 * DESIGN.md section 5 "Post-pass".  With L = 0.2126 r + 0.7152 g + 0.0722 b:
 * iteration i has step 2^i and tpt_denoise's 5x5 taps, each weighted by
 * exp(-|L(c(p)) - L(c(q))| / (sigma_lum sqrt(vbar(p) + 1e-10))) and tpt_denoise's
 * normal and depth factors, where vbar is the variance through a 3x3 binomial
 * prefilter of step 1; the colour is the weighted mean, the variance
 * sum w^2 v(q) / (sum w)^2.  A pixel whose history is shorter than min_history (N <
 * min_history, N = max(history_len_in, 1)) starts from a spatial estimate instead of
 * variance_in: the variance of L over the 7x7 window under the normal and depth
 * factors, times min_history / N.
 *   radiance_in / radiance_out / bgra_out: as tpt_denoise's.  iterations 0: radiance_out
 *     is the input bit for bit.
 *   guides: normal and depth are required, albedo only with TPT_SVGF_DEMODULATE; face
 *     and material are ignored.
 *   variance_in: nullable, W*H: the variance of the luminance of the colour the filter
 *     works on (tpt_temporal's variance_out; run both passes with or both without
 *     DEMODULATE).  Negative values count as 0.  Null: every pixel takes the spatial
 *     estimate with N = 1.
 *   history_len_in: nullable, W*H (tpt_temporal's history_len_out), only with
 *     variance_in.  Null with a variance_in: every history counts as long.
 *   variance_out: nullable, W*H: the filtered variance after the last iteration (with
 *     iterations 0 the variance the filter would start from).  May be variance_in.
 *   stats->estimated: the pixels that took the spatial estimate.
 * Inputs and outputs may be host or device memory (tpt_render's stream rule for
 * device memory); all work is complete when the call returns.  `scene` supplies the
 * device, the stream and tpt_denoise's scratch planes (48 B per pixel, and up to 52 B
 * more to stage host buffers: tpt_denoise's 44 B, the variance and the history
 * length); it need not be built.  Deterministic: no floating-point atomics.
 * Non-finite input is the caller's problem.
 * TPT_ERR_INVALID_ARG (nothing is written): null scene / radiance_in / guides / params,
 * a missing normal or depth guide, a missing albedo guide under TPT_SVGF_DEMODULATE,
 * history_len_in without variance_in, width or height <= 0, iterations outside 0..8,
 * a sigma that is not > 0, min_history outside 1..65536, an unknown flag,
 * radiance_out and bgra_out both null. */
tpt_status tpt_denoise_svgf(tpt_scene* scene, int32_t width, int32_t height, const float* radiance_in,
                            const tpt_aov* guides, const float* variance_in, const float* history_len_in,
                            const tpt_svgf_params* params, float* radiance_out, float* variance_out,
                            uint8_t* bgra_out, tpt_svgf_stats* stats);

#define TPT_UPSAMPLE_DEMODULATE 0x1   /* interpolate radiance / max(albedo, 1e-3), multiply by the full-size albedo */

typedef struct {
    float   sigma_normal;    /* > 0 */
    float   sigma_depth;     /* > 0, relative */
    int32_t flags;           /* TPT_UPSAMPLE_* */
} tpt_upsample_params;

typedef struct {
    double   kernel_ms;      /* the kernel's duration (HIP events) */
    uint64_t fallback;       /* full-size pixels without an accepted tap */
} tpt_upsample_stats;

/* Guided (joint bilateral) upsampling of a low-size radiance frame to the full size, by the
 * feature buffers of both sizes rendered from one camera (tpt_render at low_width x low_height
 * covers the same sensor as at width x height).  The pass is defined in DESIGN.md section 5
 * "Guided upsampling".  A full-size pixel takes the up to 2x2 low pixels of its bilinear
 * footprint (found in integers: the tap set is exact) that hold its own material id, each
 * weighted by its bilinear weight times tpt_denoise's normal and depth factors,
 * exp(-|dn|^2 / sigma_normal^2) exp(-dz^2 / (sigma_depth^2 max(z(p)^2, 1e-12))), relative to
 * the most similar of them, so that at least one weight survives; the output is their weighted
 * mean.  A pixel none of whose taps holds its material falls back to the plain bilinear mean of
 * the radiance as given (never demodulated) and is counted in stats->fallback.  With equal sizes,
 * the same guides and no flag the output is the input bit for bit (a -0 comes out as +0); a
 * constant low frame gives that constant bit for bit.
 *   radiance_low: low_width*low_height*3 floats, row 0 = bottom.
 *   guides_low / guides: the feature buffers at the low and at the full size: normal, depth and
 *     material are required, albedo only with TPT_UPSAMPLE_DEMODULATE; face is ignored.
 *     tpt_render_aov_path's buffers are taken unchanged, as the filters take them.
 *   radiance_out: nullable, width*height*3 floats.  bgra_out: nullable, as tpt_denoise's.  At
 *     least one of the two.
 * Inputs and outputs may be host or device memory (detected per pointer; tpt_render's stream
 * rule for device memory); all work is complete when the call returns.  `scene` supplies the
 * device, the stream and the scratch; it need not be built.  The call keeps no plane per pixel:
 * only host buffers are staged, in the buffers tpt_denoise and tpt_render_aov stage theirs in (up
 * to 48 B per full-size and 44 B per low-size pixel), and 32 KiB of counters.  Deterministic: the
 * only atomics are the integer counters of stats->fallback.  Non-finite input radiance is the
 * caller's problem.
 * TPT_ERR_INVALID_ARG (nothing is written): null scene / radiance_low / guides_low / guides /
 * params, a missing normal, depth or material guide in either set, a missing albedo guide in
 * either set under TPT_UPSAMPLE_DEMODULATE, a size <= 0, a low size larger than the full size, a
 * side above 1,048,576, a sigma that is not > 0, an unknown flag, radiance_out and bgra_out both
 * null. */
tpt_status tpt_upsample(tpt_scene* scene, int32_t low_width, int32_t low_height,
                        const float* radiance_low, const tpt_aov* guides_low,
                        int32_t width, int32_t height, const tpt_aov* guides,
                        const tpt_upsample_params* params,
                        float* radiance_out, uint8_t* bgra_out, tpt_upsample_stats* stats);

/* Tone mapping: exposure, tone curve and display encoding (DESIGN.md section 5 "Tone mapping",
 * which holds the definition in full).  The display stage behind the post-pass: every other
 * bgra_out of this header is linear radiance times 255, clamped and truncated (the reference's
 * toUChar); this one is exposed, tone-mapped, encoded and rounded.
 *
 * tpt_exposure is the adapted exposure across frames.  It belongs to a scene (its device and
 * stream), as a tpt_history does, and is destroyed before it.  It holds 2 KiB (the last
 * measured histogram) and a few words on the device. */
typedef struct tpt_exposure tpt_exposure;
tpt_status tpt_exposure_create(tpt_scene* scene, tpt_exposure** out);
/* Forget the adapted value: the next TPT_TONEMAP_AUTO call starts at its target. */
tpt_status tpt_exposure_reset(tpt_exposure* exposure);
void       tpt_exposure_destroy(tpt_exposure* exposure);
/* The 256 bin counts of the last TPT_TONEMAP_AUTO call on the handle (zeros before the first);
 * for tests and tools. */
tpt_status tpt_exposure_histogram(const tpt_exposure* exposure, uint64_t* bins256);
/* The duration of that call's measurement kernel (HIP events; 0 before the first); for tools. */
tpt_status tpt_exposure_measure_ms(const tpt_exposure* exposure, double* ms);

#define TPT_TONEMAP_AUTO    0x1    /* measure the frame's exposure (below); else scale = 2^ev */
#define TPT_TONEMAP_DITHER  0x2    /* ordered 4x4 dither before the bytes are rounded */
#define TPT_TONEMAP_LINEAR   0     /* op: y = min(x, 1) */
#define TPT_TONEMAP_REINHARD 1     /* op: extended Reinhard on luminance */
#define TPT_TONEMAP_ACES     2     /* op: ACES fit (Narkowicz 2015), per channel */
#define TPT_TRANSFER_NONE    0
#define TPT_TRANSFER_SRGB    1     /* piecewise sRGB OETF */
#define TPT_TRANSFER_GAMMA   2     /* y^(1 / gamma) */

typedef struct {
    int32_t op, transfer, flags;
    float ev;               /* stops, finite; fixed exposure, and added to the measured one under AUTO */
    float white;            /* > 0: Reinhard's white point, in exposed luminance */
    float gamma;            /* > 0: transfer 2 */
    float key;              /* > 0: AUTO brings the trimmed log-average luminance to this */
    float p_low, p_high;    /* 0 <= p_low < p_high <= 1: the share of counted pixels, by luminance, that is averaged */
    float min_ev, max_ev;   /* min_ev <= max_ev: clamp of the measured log2 scale */
    float rate;             /* (0, 1]: how far the state moves to its target per call; 1 = no adaptation */
} tpt_tonemap_params;

typedef struct {
    double   hist_ms, map_ms;             /* HIP events; hist_ms 0 without AUTO */
    float    log2_scale, scale;           /* what the map kernel used */
    float    log2_avg;                    /* the trimmed log-average, AUTO */
    uint64_t counted, dark, nonfinite;    /* AUTO; counted + dark + nonfinite == width * height */
} tpt_tonemap_stats;

/* One frame through exposure, tone curve, transfer function and rounding to bytes.
 *   Luminance L = (0.2126 r + 0.7152 g) + 0.0722 b in float, uncontracted.
 *   AUTO: a histogram of L over the frame, 256 bins of 1/8 octave over [2^-16, 2^16) taken from
 *     the float's exponent and top three mantissa bits (L < 2^-16 is `dark`, NaN `nonfinite`,
 *     L >= 2^16 bin 255); log2_avg is the mean of the bins' log2 centres over the pixels between
 *     the shares p_low and p_high of the counted ones; target = clamp(log2(key) - log2_avg,
 *     min_ev, max_ev); with an adapted `exposure` s = s' + rate (target - s'), else s = target; a
 *     frame without a counted pixel keeps s' (0 without one).  log2_scale = s + ev.
 *   Without AUTO: log2_scale = ev; `exposure` is neither read nor written.
 *   Per channel x = min(max(c 2^log2_scale, 0), 65504), NaN to 0; the op; the transfer: y in [0, 1].
 *   Bytes: floor(clamp(255 y + 0.5 + d, 0, 255)), d the 4x4 Bayer offset under DITHER, else 0.
 *   radiance_in: width*height*3 floats, row 0 = bottom.  radiance_out: nullable, the same shape,
 *     receives y; it may be radiance_in.  bgra_out: nullable, as tpt_denoise's (row 0 = top; B, G,
 *     R written, alpha untouched).  At least one of the two.
 *   exposure: nullable; with AUTO and none, the frame is measured and mapped without adaptation.
 * Pointers are host or device memory (detected per pointer; tpt_render's stream rule for device
 * memory); host buffers are staged in the buffers tpt_denoise stages its radiance and bytes in;
 * all work is complete when the call returns.  `scene` supplies the device, the stream and the
 * scratch (512 KiB of partial histograms under AUTO); it need not be built.  Deterministic: the
 * counts are integers, and the scale goes from the measurement to the map kernel in device memory.
 * TPT_ERR_INVALID_ARG (nothing is written, the exposure is left as it was): null scene /
 * radiance_in / params, both outputs null, an exposure of another scene, a size <= 0, a side
 * above 1,048,576, more than 2^31 pixels, an unknown op, transfer or flag, a parameter outside
 * the ranges of tpt_tonemap_params or NaN. */
tpt_status tpt_tonemap(tpt_scene* scene, tpt_exposure* exposure, int32_t width, int32_t height,
                       const float* radiance_in, const tpt_tonemap_params* params,
                       float* radiance_out, uint8_t* bgra_out, tpt_tonemap_stats* stats);

/* Introspection for tests: copy back the built BVH in the reference node
 * layout (bvh.cuh:52-58, 36 B/node, 2F-1 nodes) and the sorted Morton keys. */
tpt_status tpt_scene_read_bvh(tpt_scene* scene, void* nodes36, int64_t* keys);
/* The same for the resident 4-wide traversal trees, as uploaded or refitted: *n_main nodes of
 * the main tree, then *n_emit of the emissive-triangle tree (its links count from *n_main),
 * 32 floats each (inner4 layout: child k's box in floats 6k..6k+5, the four links' bits in
 * floats 24..27).  nodes: nullable; written only when cap >= *n_main + *n_emit.  After
 * tpt_scene_refit the nodes36 boxes and these are the refitted ones; the keys are the last
 * full build's. */
tpt_status tpt_scene_read_wide(tpt_scene* scene, float* nodes, int32_t cap, int32_t* n_main, int32_t* n_emit);
/* World-space vertices / normals after tpt_scene_build (n_vertices*3 each). */
tpt_status tpt_scene_read_world(tpt_scene* scene, float* wverts, float* wnorms);
/* Per-pixel RNG states after setupRandSeed for the first n pixels: 6 words
 * each {v0..v4, d}. */
tpt_status tpt_debug_rng_init(int device, uint64_t seed, uint64_t first_pixel, uint32_t n, uint32_t* states);
/* Trace n rays (origins/dirs xyz) against the built BVH: hit fid (-1 miss), t, u, v.
 * origin_fid: nullable; per ray the face it leaves (-1: none), for the render's
 * grazing test (a ray within 1e-3 of that face's plane takes the uncull'd path).
 * mode 0: closest hit in the reference's visit order (traverseBVH, path_tracer.cu:61-107);
 * 1: closest hit through the render's traversal (nearer-first, culled, 4-wide);
 * 2: any hit (shadow rays); 3: the render's two-pass direct probe -- hit = the
 * closest hit if it is an emitter, -2 if a non-emitter is closer, -1 if no emitter is hit. */
tpt_status tpt_debug_trace_rays(tpt_scene* scene, uint32_t n, const float* origins, const float* dirs,
                                const int32_t* origin_fid, int32_t mode, int32_t* hit, float* t, float* uv);
/* Known-answer evaluation of the trace kernel's own device functions, one case
 * per lane (tests pin them to the reference's headers):
 *   op 0 rayHitBBox   in 12/case (o3 d3 min3 max3)          out 2 (box_hit, min/max verdict)
 *   op 1 rayHitTriangle in 15 (o3 d3 v0_3 v1_3 v2_3)         out 4 (hit, dist, u, v)
 *   op 2 DeltaLight::sample in 16 (type color3 intensity pos3 dir3 cos_outer
 *        inv_cos_cone_diff p3)                              out 6 (dir3, radiance3)
 *   op 3 Spectrum::toUChar in 3                             out 3 (bytes as floats) */
tpt_status tpt_debug_hot_kat(int device, int32_t op, uint32_t n, const float* in, float* out);
/* Known-answer evaluation of the env paths, the parity trig and getNewDirection as the device
 * compiles them, one case per lane (tests compare them bit for bit with the CPU oracle's hooks).
 * env: the map of ops 3 and 4 (its texels and its real importance-sampling tables), null otherwise;
 * state: op 5 only, 6 words per case {v0..v4, d}, advanced in place.
 *   op 0 fsincos_2pi       in 1 (x)                        out 2 (sin, cos)
 *   op 1 atan2, double path in 2 (y, x)                     out 1
 *   op 2 acos, double path  in 1 (y)                        out 1
 *   op 3 env lookup        in 3 (dir)                      out 10 (fast column, fast row: -1 when the
 *        fp32 bounds do not decide; exact column, exact row; the lookup's rgb out of line as
 *        the variants without env IS call it; rgb inlined as the env-IS variants do)
 *   op 4 env sample        in 5 (incident-side normal3, x1, x2 in [0, 1])
 *                                                          out 7 (ok, dir3, Le cos / (pi pdf) x3:
 *        zero when not ok)
 *   op 5 getNewDirection   in 8 (d3, n3, eta, metallic)    out 5 (next3, attenuation, pdf)
 * TPT_ERR_INVALID_ARG: an unknown op, a missing env or state, an env on another device, op 4 on
 * an env whose distribution is empty (all black) or with a uniform outside [0, 1]. */
tpt_status tpt_debug_env_kat(int device, const tpt_env* env, int32_t op, uint32_t n, const float* in,
                             uint32_t* state, float* out);
/* Diagnostics: the waves per trace workgroup this build declares for a kernel family (tpt_stats.wg_waves
 * reports what a call ran): 0 one lane per pixel, 1 the same on drained launches, 2 pair mode, 3 env
 * importance sampling, 4 four lanes per pixel, 5 the reference's visit order; another family: 0 */
int32_t tpt_debug_trace_wg_waves(int32_t family);
/* Diagnostics: the per-step latency of ONE 64-lane wave walking n <= 64 closest-hit rays
 * with the render's traversal ("The drained chain"); mode 0 reads the
 * 4-wide nodes from global memory as the render does, 1 from a copy of the whole main tree
 * in LDS, 2 four lanes per ray (n <= 16: lane k of a ray's quad tests child k of each node,
 * its leaf children at once; node visits in out's first word); flags TPT_FLAG_FAST: the
 * tolerance-mode build.  out: 4 words per lane (64 lanes; per ray in mode 2): visits + leaf
 * tests of the lane, loop iterations of the wave, shader cycles of the wave's walk
 * (s_memtime), hit fid. */
tpt_status tpt_debug_step_latency(tpt_scene* scene, uint32_t n, const float* origins, const float* dirs,
                                  int32_t mode, int32_t flags, uint64_t* out);
/* Host-only: the SAH 4-wide traversal tree tpt_scene_build uploads, over n >= 2
 * leaf boxes (6 floats each, by LBVH sorted position) and emitter flags.  Writes
 * at most `cap` nodes of 32 floats (inner4 layout, device_api.hpp) and the
 * most stack entries its ordered walk can hold; returns the node count (> cap:
 * not written), or -1.  threads as in tpt_scene_set_build_threads. */
int32_t tpt_wide_tree_build(int32_t n, const float* leaf_box, const uint32_t* leaf_emit, float* nodes,
                            int32_t cap, int32_t* stack_need, int32_t threads);
/* Host-only: the levels of such a tree, which is numbered breadth-first (n_nodes nodes of 32
 * floats; id_base: the id its links give its first node, 0 for tpt_wide_tree_build's output).
 * Level l is the nodes [level_begin[l], level_begin[l + 1]) counted from the tree's first;
 * every inner child of a level-l node lies in level l + 1.  tpt_scene_refit launches one
 * kernel per level.  Returns the level count L and writes L + 1 entries when cap >= L + 1;
 * -1: null nodes, n_nodes <= 0, or nodes that are not numbered level by level. */
int32_t tpt_wide_tree_levels(const float* nodes, int32_t n_nodes, int32_t id_base, int32_t* level_begin,
                             int32_t cap);

/* Host-only: for each of n_objects the way from this frame's world back into the previous
 * one's, from the objects' local-to-world matrices then (prev16) and now (cur16; 16 floats
 * each, column-major), computed in double and rounded to float once.  out24, 24 floats per
 * object: D = M' M^-1 as three rows of four (the translation last), G = (D_lin)^-T as three
 * rows of three, the flag as an int32, two floats of padding.  Flag 1 (identity): the 16
 * floats of M' and M are bit-equal; D and G are exact unit matrices.  Flag 2 (untracked): M
 * is singular, either matrix's last row is not (0, 0, 0, 1), or an entry of D or G is not
 * finite.  Flag 0 (tracked) otherwise.  Returns the number of untracked objects, or -1 for a
 * null pointer with n_objects > 0. */
int32_t tpt_motion_matrices(uint32_t n_objects, const float* prev16, const float* cur16, float* out24);

/* ---- host-side glTF loader (mesh.cu:80-397 semantics) -------------------- */
typedef struct tpt_gltf tpt_gltf;
tpt_status tpt_gltf_load(const char* path, tpt_gltf** out);
/* Borrowed views valid until tpt_gltf_free. */
tpt_status tpt_gltf_desc(const tpt_gltf* g, tpt_scene_desc* desc, tpt_camera* camera);
/* 1 if a mesh had no material (reference reads out of bounds; we use Material()). */
int tpt_gltf_missing_material(const tpt_gltf* g);
void tpt_gltf_free(tpt_gltf* g);

#ifdef __cplusplus
}
#endif
#endif /* TPT_H */
