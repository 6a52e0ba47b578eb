// device_api.hpp -- launch entry points of the HIP kernels (host-callable).
//
// HBM layout of a built scene (see DESIGN.md "Data layout"):
//   inner[4*(F-1)] float4  internal node i: both child AABBs + child links
//       q0 = (L.min.xyz, L.max.x)  q1 = (L.max.yz, R.min.xy)
//       q2 = (R.min.z, R.max.xyz)  q3 = (bits(left), bits(right), 0, 0)
//     child ids use the reference numbering (bvh.cu:164-214): id >= F-1 is
//     the leaf at sorted position id-(F-1).  Bit 30 of every child link is
//     set when that child's subtree holds an emissive triangle; traversals
//     mask it off.
//   inner4[8*(F-1)] float4  4-wide nodes for the ordered traversal, numbered
//     breadth-first: child k box = floats 6k..6k+5 of q0..q5 (min.xyz,
//     max.xyz), q6 = child ids (-1: none; a 4-wide node id < F-1, or F-1 +
//     leaf position).  Default (wide_bvh.cpp, host): an SAH tree over the
//     LBVH's exact leaf boxes in [0, n4), then from emit_root a tree over the
//     emissive triangles alone.  Fallback
//     (non-finite boxes, or a tree deeper than the stack): the LBVH's
//     even-depth nodes, each holding its up to 4 grandchildren (a leaf child
//     stands for itself), bit 30 = emitter (ignored).
//   tri[3*F] float4    leaf slot j: (v0.xyz, bits(fid)), (e1.xyz, 0), (e2.xyz, 0) (tri_rec.hpp)
//   shade[3*F] float4  face fid: (n0.xyz, bits(mtl)), (n1.xyz, geometric unit normal .x, sign of .z in
//                      its lowest bit; NaN: none), (n2.xyz, geometric normal .y)
//   mtl[2*M] float4    (base.rgb, emission), (eta, metallic, 0, 0)
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace tpt {

struct DevLight {
    int32_t type;
    float color[3];
    float intensity;
    float pos[3];
    float dir[3];
    float cos_outer;
    float inv_cos_cone_diff;
};

constexpr int kMaxLights = 16;

struct TraceArgs {
    // scene
    const float4* inner;
    const float4* inner4;
    int32_t n4;                          // 4-wide nodes
    // Always 0 / the stack's offset (launch_trace).  k_trace's prologue still runs its staging loop
    // over 8 * lds_nodes float4 (the withdrawn "top nodes in LDS" experiment):
    // taking the loop out changes the register allocation of 21 k_trace variants (C2's among them:
    // 9 -> 16 spilled VGPRs), so it waits for a change that is measured on its own.
    int32_t lds_nodes;
    int32_t lds_nodes_offset;
    const float4* tri;
    const float4* shade;
    const float4* mtl;
    int32_t n_faces;
    int32_t n_materials;
    int32_t n_lights;
    int32_t stack_depth;                 // LDS stack slots per lane
    const DevLight* lights;
    // env (nullable)
    const uint32_t* env;                 // RGBA8 packed, row 0 = bottom
    int32_t env_w, env_h;
    // env importance sampling (A15) over blocks of is_b x is_b texels (api_scene.cpp build_env_is)
    int32_t is_b, is_bw, is_bh;          // block side; blocks per block row; block rows
    const float* is_cond;                //   block-row prefix sums [bh][bw]
    const float* is_row;                 //   block-row sums [bh]
    const float* is_marg;                //   marginal prefix over block rows [bh]
    float is_total;
    // guide tables of the two searches (exact lower_bound in few dependent loads):
    // is_guide_r[k] = lower_bound(is_marg, (k / kr) * is_total), k = 0..kr;
    // is_guide_c[by * (kc + 1) + k] = lower_bound(block row by of is_cond, (k / kc) * is_row[by])
    const int32_t* is_guide_r;
    const int32_t* is_guide_c;
    int32_t is_kr, is_kc;                // powers of two
    int32_t env_is;                      // TPT_FLAG_ENV_IS and a non-empty distribution
    // camera
    float c2w[16];
    float origin[3];                     // c2w * (0,0,0,1)
    float sensor_w, sensor_h;            // aspect*2tan(vfov/2), 2tan(vfov/2)
    float half_sw, half_sh;              // 0.5*sensor_w, 0.5*sensor_h
    float inv_w, inv_h;                  // 1/W, 1/H
    // frame
    int32_t width, height;
    int32_t band_rows, band_count, band_index, band_height;   // band_height: rows in this band
    const int32_t* band_list;            // nullable: local band k renders global band band_list[k] (explicit deal;
                                         //   only the last entry may be a short band); dispatched in list order
    unsigned long long* band_cost;       // nullable: per global band, the summed life of the waves that rendered
                                         //   it (s_memrealtime ticks, 100 MHz), for cost-balanced deals
    int32_t n_frames;                    // frames of the batch (grid z); frame f's state at f * planes * W*H
    int32_t max_depth;
    int32_t samples;                     // samples for this launch
    int32_t flags;
    int32_t refill;                      // leave the traversal loop below this many active lanes
    int32_t leaf_kb;                     // run the parked triangle tests once this many lanes are blocked
    int32_t boxes_finite;                // all node boxes finite: min/max slab test is exact
    int32_t any_emitter;                 // some triangle emits (else a direct probe adds nothing)
    int32_t emit_root;                   // inner4 id of the emissive-triangle tree (-1: none)
    // 1: every material's baseColor component is finite, has a clear sign bit and is at most
    // kPruneColorCap (trace_variant.hpp), so the unwind may skip levels that provably give +0
    // (trace.hip "Pruned unwind").  (Fills the padding before emit_box: no other field moves.)
    int32_t unwind_prune;
    // Boxes enclosing every emissive triangle's leaf box (the emissive tree
    // root's child boxes, overlapping ones merged): (lo.xyz, 0), (hi.xyz, 0) per
    // box.  A direct probe whose line misses all of them by a margin can hit no
    // emitter and is resolved in the shading pass (trace.hip probe_misses_emitters)
    float4 emit_box[8];
    int32_t n_emit_box;                  // 0: no pre-test (no emissive tree, or non-finite boxes)
    const float4* sliver_groups;         // 2 per group: (lo.xyz, first), (hi.xyz, count) (trace.hip "Culling")
    const float4* sliver_list;           // 2 per sliver: (exact leaf box lo.xyz, position | emissive << 30), (hi.xyz, 0)
    int32_t n_sliver_groups;             // 0: no sliver triangles
    float cull_eps;                      // absolute position slack of the t-culls (trace.hip "Culling")
    int32_t graze;                       // 1: rays leaving a face within 1e-3 of its plane skip the culls (grazing())
    int32_t pair;                        // 1: pair mode (two lanes per pixel, shadow rays on the side lane)
    int32_t drained;                     // 1: the launch cannot fill the chip (latency-oriented DRAIN variants)
    int32_t quad;                        // 1: four lanes per pixel, each node visit split over them (k_trace QUAD)
    int32_t xcd_run;                     // > 0: workgroup tiles dealt to XCDs in runs of this many (k_trace)
    int32_t xcd_rot;                     // the runs' XCD rotation of this launch (its chunk of the set's spp)
    int32_t lds_rec_offset;              // set by launch_trace: byte offset of the record region
    int32_t rec_lds_levels;              // set by launch_trace: path-record levels held in LDS
    int32_t stack_lds_slots;             // set by launch_trace: stack slots held in LDS (rest private)
    int32_t lds_stack_offset;            // set by launch_trace: byte offset of the stack region
    int32_t lds_mtl_offset;              // set by launch_trace: byte offset of the material table
    int32_t mtl_in_lds;                  // set by launch_trace: material table copied to LDS
    // per-pixel state (SoA over W*H pixels)
    uint32_t* rng;                       // 6 planes: v0..v4, d
    float* accum;                        // 3 planes: r, g, b (running totalRad)
    unsigned long long* counters;        // [0] trav [1] inner [2] leaf [3] shade [4] overflow [5] wide
    unsigned long long* debug_waves;     // phase-profiling builds: 8 words per wave (null: off)
    // Listed launch (tpt_render_adaptive; nullable, device memory): n_tiles 16x16-pixel tiles, each packed
    // tx | ty << 16, rendered in list order by a one-dimensional grid.  The frame is whole then: no bands,
    // band list or band_cost, one frame, no XCD runs.  (Last in the struct: no other field moves.)
    const uint32_t* tile_list;
    int32_t n_tiles;
    // Run-ahead (trace_variant.hpp trace_runs_ahead; variants compiled without it ignore both).
    // ahead_max: the samples the same set's later launches will still give these pixels (0: its
    // last launch, or off).  credit: nullable, one int per pixel and frame, indexed like one RNG
    // plane: the samples of this launch's quota the pixel has already run (read), those of the
    // later launches' it ran here (written).  Null: every lane runs exactly `samples`.
    // (Appended: no other field moves; ahead_max fills the padding behind n_tiles.)
    int32_t ahead_max;
    int32_t* credit;
};

struct ResolveArgs {
    const float* accum;
    float* radiance;                     // device, W*H*3 (nullable)
    uint8_t* bgra;                       // device, W*H*4 (nullable)
    int32_t width, height;
    int32_t band_rows, band_count, band_index, band_height;
    const int32_t* band_list;            // as TraceArgs
    int32_t spp;
};

// rng.hip
hipError_t launch_rng_init(const uint32_t* jumps, uint64_t seed, int32_t width, int32_t band_rows,
                           int32_t band_count, int32_t band_index, const int32_t* band_list, int32_t band_height,
                           int32_t height, uint32_t* rng, hipStream_t s);
hipError_t launch_rng_init_linear(const uint32_t* jumps, uint64_t seed, uint64_t first, uint32_t n,
                                  uint32_t* states_aos, hipStream_t s);

// build.hip
struct BuildBuffers {
    int32_t n_faces, n_vertices, n_objects, n_materials;
    const uint32_t* indices;
    const float* vertices;
    const float* normals;
    const int2* lut;
    const float* vert_trans;
    const float* normal_trans;
    const float4* mtl;
    float* wverts;
    float* wnorms;
    // temporaries
    unsigned long long* keys;
    unsigned long long* keys_sorted;
    uint32_t* fids;
    uint32_t* fids_sorted;
    float* leaf_box;                     // 6 per face (min.xyz, max.xyz) by fid
    int2* children;                      // F-1
    uint32_t* parent;                    // 2F-1
    float* node_box;                     // 6 per node (2F-1)
    uint32_t* flags;                     // F-1
    uint32_t* max_depth;                 // 3: deepest leaf, non-finite inner-box flag, 4-wide node count
    unsigned long long* bfs_keys;        // F-1: (level, id) keys of the 4-wide nodes
    unsigned long long* bfs_keys_sorted;
    uint32_t* bfs_ids;                   // F-1
    uint32_t* bfs_ids_sorted;
    uint32_t* bfs_newid;                 // F-1: binary id -> breadth-first 4-wide id
    uint32_t* emit;                      // 2F-1: subtree holds an emissive triangle
    void* sort_tmp;
    size_t sort_tmp_bytes;
    // outputs
    float4* inner;
    float4* inner4;
    float4* tri;
    float4* shade;
    void* nodes36;                       // reference layout (2F-1) * 36 B
    uint32_t out_max_depth;              // deepest leaf (root = 0), set by launch_build
    uint32_t out_boxes_finite;           // 1: every inner-node child box is finite
    uint32_t out_n4;                     // 4-wide nodes (breadth-first prefix of inner4)
};
// launch_build fails with hipErrorInvalidValue (out_max_depth >= kMaxLbvhDepth)
// when a leaf's parent chain does not reach the root within this many steps
constexpr uint32_t kMaxLbvhDepth = 4096;
hipError_t build_sort_tmp_bytes(int32_t n, size_t* bytes);
hipError_t launch_build(BuildBuffers& b, hipStream_t s);
// Culling exactness inputs (trace.hip "Culling"), per leaf position of the packed
// triangles: sliver[p] = 1 when sin of the angle at v0 between e1 and e2 is below
// 1e-3, and *coord_max (zeroed by the caller) = the bits of the largest
// |coordinate| of any vertex as a double (positive doubles order as integers).
hipError_t launch_sliver_scan(const float4* tri, int32_t n, uint8_t* sliver, unsigned long long* coord_max,
                              hipStream_t s);
// Refit (tpt_scene_refit): what launch_build left resident -- fids_sorted, children, parent, the
// node depths in `flags`, emit, the links of inner4 -- stays; wverts / wnorms (zeroed by the
// caller), leaf_box, node_box, inner, the boxes of inner4, tri, shade and nodes36 are
// recomputed from vertices and the matrices.  max_depth[1] is nonzero afterwards when a face
// has a non-finite world vertex or an inner-node child box is not finite.
struct RefitPlan {
    uint32_t tree_depth;                 // the LBVH's deepest leaf (BuildBuffers::out_max_depth of the build)
    // Level l of a 4-wide tree is the inner4 ids [lv[l], lv[l + 1]) (tpt_wide_tree_levels, plus
    // the tree's first id); n_lv levels.  The emissive tree may have none (n_lv_emit = 0).
    const int32_t* lv_main;
    int32_t n_lv_main;
    const int32_t* lv_emit;
    int32_t n_lv_emit;
};
// *launches is advanced by the kernels launched
hipError_t launch_refit(BuildBuffers& b, const RefitPlan& p, int32_t* launches, hipStream_t s);
// out[0] = the sum over the main tree's n_main nodes of their child boxes' areas (double, a
// fixed order), out[1] = the area of the union of the root's child boxes; terms: n_main doubles
hipError_t launch_wide_cost(const float4* inner4, int32_t n_main, double* terms, double* out, int32_t* launches,
                            hipStream_t s);

// wavefront.hip: the wavefront / ray-queue variant (TPT_FLAG_WAVEFRONT).  The
// queues are split into kWfShards shards (one per XCD) of shard_cap entries.  Slots
// run pixels' sample chains; their state lives here between iterations, and the
// rays move through two ping-pong queues (2 float4 each: origin + slot, direction
// + flags) with one hit record (t, u, v, fid code) per queue position.
constexpr int kWfShards = 8;
constexpr int kWfCtlStride = 1024;                     // words between control words (4 KiB)
constexpr int kWfCtlWords = (4 * kWfShards + 1) * kWfCtlStride;
struct WfArgs {
    TraceArgs t;                         // scene, camera, frame, RNG/accumulator planes, counters
    int32_t n_slots;                     // concurrent paths (slots)
    int32_t state_words;                 // 16, or 32 with delta lights / env IS / reference order
    int32_t rec_words;                   // path-record words per bounce (2 or 5)
    int32_t ordered;                     // 0: the reference's visit order (TPT_FLAG_REF_ORDER)
    uint32_t* st0;                       // path state beside queue 0's entries: state_words per entry
    uint32_t* st1;                       // ... beside queue 1's
    float* rec;                          // n_slots * max_depth * rec_words
    float4* q_ray0;                      // 2 * kWfShards * shard_cap float4
    float4* q_ray1;                      // 2 * kWfShards * shard_cap float4
    float4* q_hit;                       // kWfShards * shard_cap float4
    uint32_t* ctl;                       // kWfCtlWords: shard sizes and fetch heads of both queues, claims
    int32_t shard_cap;                   // entries per shard: ceil(n_slots / 256 / kWfShards) * 256
    int32_t n_claims;                    // claim ids (k_trace dispatch order; those outside the band are skipped)
    int32_t refill;                      // k_wf_trace: a wave runs its pass (hits out, rays in) below this many
                                         //   traversing lanes
    int32_t chunk;                       // k_wf_trace: queue entries a wave takes per global atomic
    int32_t batch;                       // iterations enqueued between two checks of the queue size
    int32_t logic_blocks, trace_blocks;  // grid sizes (both kernels are grid-stride / persistent)
    int32_t it;                          // set per launch: iteration (queue it & 1 is consumed)
    int32_t stack_lds_slots, lds_stack_offset, lds_bytes;   // set by launch_wavefront
};
// Runs every iteration until the queues are empty (stream-ordered; the caller
// synchronises).  h_count: 2 * kWfShards words of pinned host memory; ev: 2 events.
hipError_t launch_wavefront(WfArgs w, uint32_t* h_count, hipEvent_t ev[2], int32_t* iterations, hipStream_t s);

// trace.hip
// shape (optional, kTraceShapeWords ints): what the launch ran as -- the waves per
// workgroup of the variant's family (WGW), the workgroups of that size and LDS the
// runtime says a CU holds, the number that fills the CU's wave slots (4 SIMDs x the
// variant's waves per SIMD / WGW; the LDS layout shrinks until it is met), the
// workgroup's LDS bytes, its LDS stack slots and record levels
constexpr int kTraceShapeWords = 6;
hipError_t launch_trace(const TraceArgs& a, hipStream_t s, int32_t* shape = nullptr);
bool trace_quad_fits(const TraceArgs& a);   // lanes_per_pixel 4: one-lane records, the quads' stacks fit in LDS
bool trace_args_run_ahead(const TraceArgs& a);   // the variant launch_trace picks for `a` is compiled with run-ahead
int trace_family_wgw(int family);           // tpt_debug_trace_wg_waves
int trace_waves_per_simd();                 // the one-lane variants' __launch_bounds__ waves per SIMD
hipError_t launch_trace_ptr(const void* a, hipStream_t s, int32_t* shape);   // a: const TraceArgs*
// lone-wave step latency probe (tpt_debug_step_latency), a: const TraceArgs*
hipError_t launch_step_latency_ptr(const void* a, uint32_t n, const float* o, const float* d, int nodes_lds,
                                   unsigned long long* out, hipStream_t s);
hipError_t launch_resolve(const ResolveArgs& a, hipStream_t s);

// adaptive.hip: the tile error estimate and the per-tile resolve of tpt_render_adaptive (DESIGN.md
// section 5 "Adaptive sampling").  Tiles are 16x16 pixels, packed tx | ty << 16 like TraceArgs::tile_list.
struct TileErrorArgs {
    const float* accum;                  // 3 planes of W*H sums (TraceArgs::accum)
    float* snapshot;                     // 3 planes: the sums when the listed tiles had n / 2 samples
    const uint32_t* tile_list;           // n_tiles entries
    float* tile_error;                   // tiles_y * tiles_x, row 0 = bottom; listed tiles' entries are written
    int32_t n_tiles;
    int32_t width, height, tiles_x;
    int32_t n;                           // samples the listed tiles hold now (even)
    int32_t snapshot_only;               // 1: only copy the listed tiles' sums to the snapshot
};
hipError_t launch_tile_error(const TileErrorArgs& a, hipStream_t s);
struct ResolveTilesArgs {
    const float* accum;
    const int32_t* tile_spp;             // tiles_y * tiles_x: the samples each tile holds
    float* radiance;                     // as ResolveArgs
    uint8_t* bgra;
    int32_t width, height, tiles_x;
};
hipError_t launch_resolve_tiles(const ResolveTilesArgs& a, hipStream_t s);
// KAT kernel over the trace kernel's device functions (tpt_debug_hot_kat)
hipError_t launch_hot_kat(int op, uint32_t n, const float* in, float* out, hipStream_t s);
hipError_t launch_trace_rays(const TraceArgs& a, uint32_t n, const float* o, const float* d, const int32_t* ofid,
                             int mode, int32_t* hit, float* t, float* uv, hipStream_t s);

// post.hip: first-hit feature buffers (tpt_render_aov) and the a-trous denoiser (tpt_denoise)
struct AovArgs {                         // device pointers, each nullable; W*H pixels, row 0 = bottom
    float* albedo;                       // 3 per pixel
    float* normal;                       // 3 per pixel
    float* depth;
    int32_t* face;
    int32_t* material;
};
// a: the scene, the camera constants, width, height, inv_w, inv_h (whole frame; bands do not apply)
hipError_t launch_aov(const TraceArgs& a, const AovArgs& o, hipStream_t s);

// post.hip k_aov_path: the same continued through perfect mirrors (tpt_render_aov_path)
struct AovPathArgs {
    int32_t* bounces;                    // nullable, W*H: mirrors followed
    int32_t max_bounces;
    unsigned long long* followed;        // kTemporalSlots counters, kTemporalSlotStride words apart (zeroed by the
                                         //   caller): their sum = pixels with bounces > 0
    unsigned long long* deepest;         // as many, as far apart (zeroed): their maximum = the largest bounces
};
hipError_t launch_aov_path(const TraceArgs& a, const AovArgs& o, const AovPathArgs& p, hipStream_t s);
// post.hip k_aov_path_points: the same, and where each path ended (tpt_render_aov_path_points).
// points: W*H*3, never null: the terminal hit point, or the last ray's direction on a miss
hipError_t launch_aov_path_points(const TraceArgs& a, const AovArgs& o, const AovPathArgs& p, float* points, hipStream_t s);

struct DenoiseArgs {                     // pack (inputs -> planes) and resolve (plane -> outputs)
    const float* radiance_in;            // pack: W*H*3
    const float* albedo;                 // W*H*3 (read when demodulate)
    const float* normal;                 // pack: W*H*3
    const float* depth;                  // pack: W*H
    float4* color0;                      // pack writes it (rgb, 0); resolve reads the last iteration's plane here
    float4* guide;                       // pack: (n.xyz, z)
    float* radiance_out;                 // resolve: nullable, W*H*3, row 0 = bottom
    uint8_t* bgra;                       // resolve: nullable, W*H*4, row 0 = top, alpha untouched
    size_t npix;
    int32_t width, height;
    int32_t demodulate;
};
struct AtrousArgs {                      // one iteration: dst = filter(src) at this step
    const float4* src;
    const float4* guide;
    float4* dst;
    int32_t width, height;
    int32_t step;                        // 2^i
    float inv_sc2;                       // 1 / sigma_c,i^2
    float inv_sn2;                       // 1 / sigma_n^2
    float sz2;                           // sigma_z^2
};
hipError_t launch_denoise_pack(const DenoiseArgs& a, hipStream_t s);
// use_lds: steps 1 and 2 through the LDS-staged kernel (bit-identical to the direct one)
hipError_t launch_atrous(const AtrousArgs& a, bool use_lds, hipStream_t s);
hipError_t launch_denoise_resolve(const DenoiseArgs& a, hipStream_t s);

// post.hip: temporal reprojection and accumulation (tpt_temporal; DESIGN.md section 5
// "Post-pass").  The state is three float4 planes per pixel, in two sets that ping-pong:
//   plane 0 = (accumulated colour rgb, history length N)
//   plane 1 = (normal xyz, depth)
//   plane 2 = (luminance moments M1, M2, bits(material id), 0)
struct TemporalArgs {
    // the current camera, as TraceArgs holds it (k_aov's pixel-centre ray)
    float c2w[16];
    float origin[3];
    float sensor_w, sensor_h, half_sw, half_sh;
    float inv_w, inv_h;
    // the previous call's camera: inverse of its c2w (column-major; double, rounded to
    // float), its origin and sensor
    float prev_inv[16];
    float prev_origin[3];
    float prev_sensor_w, prev_sensor_h, prev_half_sw, prev_half_sh;
    int32_t has_prev;                    // 0: no state (after create / reset): every pixel disoccluded
    int32_t width, height;
    int32_t demodulate;
    int32_t tiles;                       // 1: 16x16 tiles (8x8 per wave) instead of 64-pixel row segments
    float alpha, depth_tol, normal_min, max_history;
    // this frame (device pointers, row 0 = bottom)
    const float* radiance_in;            // W*H*3
    const float* albedo;                 // W*H*3 (read when demodulate)
    const float* normal;                 // W*H*3
    const float* depth;                  // W*H
    const int32_t* material;             // W*H
    const float4* prev[3];               // the previous state (read, gathered)
    float4* next[3];                     // the new state (written at the lane's own pixel)
    float* radiance_out;                 // nullable, W*H*3; may be radiance_in
    float* variance_out;                 // nullable, W*H
    float* history_out;                  // nullable, W*H
    uint8_t* bgra;                       // nullable, W*H*4, row 0 = top, alpha untouched
    unsigned long long* reprojected;     // kTemporalSlots counters, kTemporalSlotStride words apart (zeroed by the
                                         //   caller): their sum = pixels that found history
};
constexpr int kTemporalSlots = 256;
constexpr int kTemporalSlotStride = 16;  // 128 B: one counter per cache line

// post.hip: what the motion-aware variant (tpt_temporal_motion) reads and writes on top of
// TemporalArgs.  A record is tpt_motion_matrices' 24 floats, read as six float4:
//   0..2 = the rows of D (D[r][0..2], translation), 3..5 = G row-major, then the flag's bits
//   (kMotionTracked / kMotionIdentity / kMotionUntracked) and two words of padding.
struct MotionArgs {
    const int32_t* face;                 // W*H: this frame's face ids (-1 on a miss)
    const int32_t* face_object;          // n_faces: the object whose lut interval holds the face
    const float4* records;               // 6 float4 per object
    float* motion_out;                   // nullable, W*H*2
    int32_t n_faces;
};
constexpr int kMotionRecordFloats = 24;
constexpr int32_t kMotionTracked = 0, kMotionIdentity = 1, kMotionUntracked = 2;

// post.hip: what the pass on mirror-path guides (tpt_temporal_path) reads and writes on top of
// TemporalArgs, whose guides are then tpt_render_aov_path's.  The bounce count k is kept as its
// integer bits in the fourth word of state plane 2 (every other variant of k_temporal writes 0.0f
// there: k = 0); the terminal points are a fourth state plane per set, (P.xyz, 0), written and
// gathered by k > 0 lanes only.
struct TemporalPathArgs {
    const int32_t* bounces;              // W*H: this frame's mirrors followed
    const float* points;                 // W*H*3: this frame's terminal points / last directions
    const float4* prev_points;           // the previous state's plane 3 (gathered where k > 0)
    float4* next_points;                 // the new state's plane 3 (written where k > 0)
    float point_tol;                     // > 0, in pixel footprints
};

// post.hip: what the variant that follows deforming meshes (tpt_temporal_deform) reads and writes
// on top of TemporalArgs: the scene's topology and world buffers as they are now, and the
// history's snapshot of the world buffers as they were at the previous call.
struct DeformArgs {
    const int32_t* face;                 // W*H: this frame's face ids (-1 on a miss)
    const uint32_t* indices;             // 3 per face
    const float* wverts;                 // 3 per vertex: the scene's world positions
    const float* wnorms;                 // 3 per vertex: its world normals
    const float* prev_wverts;            // the snapshot's positions (read only where snap_valid)
    const float* prev_wnorms;            // the snapshot's normals
    float* motion_out;                   // nullable, W*H*2
    int32_t n_faces;
    int32_t snap_valid;                  // 0: the snapshot is not the previous call's: hit pixels are disoccluded
};

// post.hip: history clipping (tpt_history_set_clip; DESIGN.md section 5 "History clipping").
// k_clip_box writes, per pixel, the box of the colours the temporal kernel accumulates over the
// pixel's similar neighbours as two float4 planes: (lo.rgb, n) and (hi.rgb, 0), n the taps
// counted; n < 4 gives lo = -inf, hi = +inf.  It reads the temporal call's own inputs.
struct ClipBoxArgs {
    int32_t width, height;
    int32_t radius;                      // 1..3: the window is (2 radius + 1)^2 pixels
    int32_t demodulate;
    float depth_tol, normal_min;         // the temporal call's own
    float gamma;                         // half-width of the box in standard deviations
    const float* radiance_in;            // W*H*3
    const float* albedo;                 // W*H*3 (read when demodulate)
    const float* normal;                 // W*H*3
    const float* depth;                  // W*H
    const int32_t* material;             // W*H
    const int32_t* bounces;              // nullable, W*H: tpt_temporal_path's k, compared as well
    float4* lo;                          // (lo.rgb, n)
    float4* hi;                          // (hi.rgb, 0)
    unsigned long long* boxed;           // kTemporalSlots counters: pixels with n >= 4
};
hipError_t launch_clip_box(const ClipBoxArgs& a, hipStream_t s);

// What the clipped temporal kernels take on top of their twins' arguments: the two planes, the
// cap on a clipped pixel's history length and the counter of the pixels whose history the clip
// moved.
struct ClipArgs {
    const float4* lo;
    const float4* hi;
    float clip_history;
    unsigned long long* clipped;         // kTemporalSlots counters, as TemporalArgs::reprojected
};
// The temporal kernel that takes the arguments given: at most one of mo, pa and de
// (hipErrorInvalidValue otherwise; none: tpt_temporal's), and cl where the history is clipped.
hipError_t launch_temporal(const TemporalArgs& a, const MotionArgs* mo, const TemporalPathArgs* pa, const DeformArgs* de,
                           const ClipArgs* cl, hipStream_t s);

// post.hip: the variance-guided a-trous filter (tpt_denoise_svgf; DESIGN.md section 5
// "Post-pass").  tpt_denoise's planes, the colour plane's fourth component carrying the
// variance: colour = (r, g, b, v), guide = (n.xyz, z).
struct SvgfArgs {                        // pack (inputs -> planes), estimate (plane -> plane), resolve (plane -> outputs)
    const float* radiance_in;            // pack: W*H*3; resolve reads it again when passthrough
    const float* albedo;                 // W*H*3 (read when demodulate)
    const float* normal;                 // pack: W*H*3
    const float* depth;                  // pack: W*H
    const float* variance_in;            // pack: nullable, W*H; null: every pixel takes the spatial estimate, N = 1
    const float* history_len;            // estimate: nullable, W*H; null with a variance_in: no pixel is short
    const float4* src;                   // estimate, resolve: the plane read
    float4* dst;                         // pack, estimate: the plane written
    float4* guide;                       // pack writes it, estimate reads it
    float* radiance_out;                 // resolve: nullable, W*H*3, row 0 = bottom
    float* variance_out;                 // resolve: nullable, W*H
    uint8_t* bgra;                       // resolve: nullable, W*H*4, row 0 = top, alpha untouched
    unsigned long long* estimated;       // estimate: kTemporalSlots counters, kTemporalSlotStride words apart
                                         //   (zeroed by the caller): their sum = pixels that took the estimate
    size_t npix;
    int32_t width, height;
    int32_t demodulate;
    int32_t passthrough;                 // resolve: radiance_out = radiance_in bit for bit (iterations 0)
    float min_history;
    float inv_sn2;                       // 1 / sigma_n^2
    float sz2;                           // sigma_z^2
};
struct SvgfFilterArgs {                  // one iteration: dst = filter(src) at this step
    const float4* src;
    const float4* guide;
    float4* dst;
    int32_t width, height;
    int32_t step;                        // 2^i
    float sigma_lum;
    float inv_sn2;                       // 1 / sigma_n^2
    float sz2;                           // sigma_z^2
};
hipError_t launch_svgf_pack(const SvgfArgs& a, hipStream_t s);
hipError_t launch_svgf_estimate(const SvgfArgs& a, hipStream_t s);
// use_lds: steps 1 and 2 through the LDS-staged kernel (bit-identical to the direct one)
hipError_t launch_svgf_filter(const SvgfFilterArgs& a, bool use_lds, hipStream_t s);
hipError_t launch_svgf_resolve(const SvgfArgs& a, hipStream_t s);

// post.hip: guided upsampling (tpt_upsample; DESIGN.md section 5 "Guided upsampling"): the low-size
// frame and its guides are gathered (four taps per full-size pixel), the full-size guides read and
// the outputs written at the lane's own pixel.  Device pointers, row 0 = bottom.
struct UpsampleArgs {
    const float* radiance_low;           // wl*hl*3
    const float* albedo_low;             // wl*hl*3 (read when demodulate)
    const float* normal_low;             // wl*hl*3
    const float* depth_low;              // wl*hl
    const int32_t* material_low;         // wl*hl
    const float* albedo;                 // W*H*3 (read when demodulate)
    const float* normal;                 // W*H*3
    const float* depth;                  // W*H
    const int32_t* material;             // W*H
    float* radiance_out;                 // nullable, W*H*3
    uint8_t* bgra;                       // nullable, W*H*4, row 0 = top, alpha untouched
    unsigned long long* fallback;        // kTemporalSlots counters, kTemporalSlotStride words apart (zeroed by the
                                         //   caller): their sum = pixels without an accepted tap
    int32_t low_width, low_height;       // 1 <= wl <= W, 1 <= hl <= H
    int32_t width, height;
    int32_t demodulate;
    float inv_sn2;                       // 1 / sigma_n^2
    float sz2;                           // sigma_z^2
};
hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t s);

// tonemap.hip: exposure, tone curve and display encoding (tpt_tonemap; DESIGN.md section 5 "Tone
// mapping").  The exposure lives in device memory between the measuring kernels and the map kernel.
struct ExposureBlock {                   // a tpt_exposure's device state, or the scene's for a call without one
    double s;                            // the adapted log2 scale (meaningful where the host says so)
    float log2_scale, scale;             // what the last AUTO call's map kernel used
    float log2_avg;
    float pad;
    unsigned long long counted, dark, nonfinite;
    unsigned long long hist[256];        // the last AUTO call's histogram
};
constexpr int kHistMaxBlocks = 512;      // the cap of the histogram kernel's grid: 2 workgroups of 256 lanes per CU
constexpr int kHistRowWords = 256;       // a workgroup's row of the partials; the rows are followed by one
                                         //   word per workgroup, its NaN count
struct HistArgs {
    const float* radiance;               // W*H*3
    size_t npix;
    uint32_t* partials;                  // kHistMaxBlocks * kHistRowWords + kHistMaxBlocks words
    int32_t blocks;                      // the grid: min(kHistMaxBlocks, ceil(npix / 256))
};
struct MeasureArgs {
    const uint32_t* partials;
    int32_t blocks;
    size_t npix;
    ExposureBlock* block;
    int32_t has_state;                   // block->s is the state s'
    double p_low, p_high, key, min_ev, max_ev, rate, ev;   // tpt_tonemap_params', widened
};
struct TonemapArgs {
    const float* radiance_in;            // W*H*3, row 0 = bottom
    float* radiance_out;                 // nullable, W*H*3; may be radiance_in
    uint8_t* bgra;                       // nullable, W*H*4, row 0 = top, alpha untouched
    const ExposureBlock* block;          // AUTO: the scale is block->scale; null: `scale`
    float scale;
    int32_t width, height;
    int32_t op, transfer, dither;
    float white2;                        // white^2
    float inv_gamma;                     // 1 / gamma
};
int hist_blocks(size_t npix);
hipError_t launch_histogram(const HistArgs& a, hipStream_t s);
hipError_t launch_measure(const MeasureArgs& a, hipStream_t s);
hipError_t launch_tonemap(const TonemapArgs& a, hipStream_t s);

}  // namespace tpt

// The tolerance-mode build of trace.hip (TPT_FLAG_FAST; Makefile trace_fast.hip.o):
// the same kernels in namespace tpt_fast, reached with a tpt::TraceArgs.
namespace tpt_fast {
hipError_t launch_trace_ptr(const void* a, hipStream_t s, int32_t* shape);
hipError_t launch_step_latency_ptr(const void* a, uint32_t n, const float* o, const float* d, int nodes_lds,
                                   unsigned long long* out, hipStream_t s);
}
