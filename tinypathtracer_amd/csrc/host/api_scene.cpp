// api_scene.cpp -- the scene and env handles of the C-ABI: tpt_scene_create, the
// (asynchronous) build with its host trees, the refit that keeps them
// (tpt_scene_refit), tpt_env_create / tpt_env_load.
//
// Replaces the reference's Scene::copySceneToDevice (src/mesh.cu:309-397).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <system_error>

#include "../common/rng.hpp"
#include "../common/tri_rec.hpp"
#include "api_internal.hpp"

namespace {

constexpr float kInfF = __builtin_huge_valf();

// A15 re-derivation (env_light.cu:10-54 intends a 2-D piecewise-constant
// distribution; its weight uses theta for sin(theta), its normalisation races
// across blocks and its row orientation is the reverse of Vec2UV).  Here the
// distribution is piecewise constant over blocks of B x B texels (B = 1 for
// maps up to 2^17 texels; doubled until the block grid has at most 2^17 cells,
// so the tables stay L2-resident: 2048 x 1024 -> B = 4, 512 x 256 blocks,
// 0.5 MB): a block's weight is the sum over its texels of luma * sin(theta at
// the texel row's centre), rows iy = 0 (bottom) .. h-1 as the lookup reads them
// (v = 1 - acos(y)/pi), texel rows then columns, then sequential float prefix
// sums per block row and over block rows -- the oracle (env_is_build) builds
// the same tables with the same operations.  A sample picks a block by the two
// CDFs and a point uniformly inside it (trace.hip env_is_sample).
int env_is_block(int w, int h) {
    int b = 1;
    while ((long long)((w + b - 1) / b) * (long long)((h + b - 1) / b) > (1ll << 17)) b *= 2;
    return b;
}
void build_env_is(const uint8_t* rgba, int w, int h, int b, std::vector<float>& cond, std::vector<float>& row,
                  std::vector<float>& marg, float& total) {
    const int bw = (w + b - 1) / b, bh = (h + b - 1) / b;
    cond.resize((size_t)bw * bh);
    row.resize(bh);
    marg.resize(bh);
    std::vector<float> sw(h);
    for (int iy = 0; iy < h; ++iy) {
        const float theta = tpt::kPi * (1.0f - ((float)iy + 0.5f) / (float)h);
        float cw;
        tpt::fsincos_2pi(theta, sw[iy], cw);
    }
    float acc_rows = 0.0f;
    for (int by = 0; by < bh; ++by) {
        float acc = 0.0f;
        for (int bx = 0; bx < bw; ++bx) {
            float wb = 0.0f;
            for (int iy = by * b; iy < std::min(by * b + b, h); ++iy)
                for (int ix = bx * b; ix < std::min(bx * b + b, w); ++ix) {
                    const uint8_t* px = rgba + 4 * ((size_t)iy * w + ix);
                    const float luma = (0.2126f * (float)px[0] + 0.7152f * (float)px[1]) + 0.0722f * (float)px[2];
                    wb = wb + luma * sw[iy];
                }
            acc = acc + wb;
            cond[(size_t)by * bw + bx] = acc;
        }
        row[by] = acc;
        acc_rows = acc_rows + acc;
        marg[by] = acc_rows;
    }
    total = acc_rows;
}

// Guide table of a nondecreasing prefix array a[0, n) with last entry `total`:
// g[k] = lower_bound(a, fl((k / K) * total)) for k = 0..K (trace.hip
// lower_bound_guided).  The thresholds are computed in float exactly as the
// kernel's t = x * total is, so the guided search returns the plain search's index.
void build_guide(const float* a, int n, float total, int K, int32_t* g) {
    const float inv = 1.0f / (float)K;   // exact: K is a power of two
    int i = 0;
    for (int k = 0; k <= K; ++k) {
        const float thr = ((float)k * inv) * total;
        while (i < n - 1 && a[i] < thr) ++i;
        g[k] = i;
    }
}

int pow2_at_least(int n) {
    int k = 1;
    while (k < n && k < (1 << 20)) k <<= 1;
    return k;
}

// TPT_BUILD_TIMING=1: per-phase wall times of tpt_scene_build on stderr
struct PhaseClock {
    bool on;
    std::chrono::steady_clock::time_point t;
    explicit PhaseClock(bool on_) : on(on_), t(std::chrono::steady_clock::now()) {}
    void mark(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "tpt_scene_build %-10s %8.3f ms\n", what,
                     std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

void build_host_trees(HostTrees& j) {
    PhaseClock clk(j.timing);
    const size_t n = j.n;
    const int leaf_base = (int)n - 1;
#ifdef TPT_WIDE_TREE_LBVH
    const bool sah = false;   // A/B builds: keep the LBVH's even-depth view
#else
    const bool sah = true;
#endif
    try {
        if (sah) {
            // SAH 4-wide traversal tree over the LBVH's exact leaf boxes (wide_bvh.cpp)
            std::vector<int> all(n);
            for (size_t p = 0; p < n; ++p) all[p] = (int)p;
            j.n4 = tpt::build_wide_sah(all, j.lbox, j.lemit, leaf_base, 0, j.w4, &j.need, j.prm);
        }
        clk.mark("sah");
        // The direct probe's first pass (closest emissive hit, trace.hip
        // TM_EMIT) walks a tree over the emissive triangles alone, appended
        // after the main tree's nodes: same exact leaf boxes and positions, so
        // the same hit as the emitter-filtered walk of the whole tree.
        std::vector<int> em;
        for (size_t p = 0; p < n; ++p)
            if (j.lemit[p]) em.push_back((int)p);
        if (!em.empty())
            j.ne4 = tpt::build_wide_sah(em, j.lbox, j.lemit, leaf_base, j.base(), j.e4, &j.eneed, j.prm);
        clk.mark("emit_tree");
    } catch (const std::bad_alloc&) {
        j.st = TPT_ERR_OOM;
        j.msg = "traversal tree build: host allocation failed";
    } catch (const std::exception& ex) {
        j.st = TPT_ERR_HIP;
        j.msg = std::string("traversal tree build: ") + ex.what();
    }
}

// The direct-probe pre-test's boxes (trace.hip probe_misses_emitters): the
// child boxes of the emissive tree's root node (4-wide layout, wide_bvh.cpp;
// they enclose every emissive triangle's leaf box), with a pair merged into
// its union while the union's surface area is at most the pair's summed areas
// (heavily overlapping boxes, e.g. the two triangles of one quad light, cost
// a test each for nothing).  Writes lo.xyz, hi.xyz per box and returns the box
// count (0: a non-finite box, no pre-test).
float box_area(const float* b) {
    const float x = b[3] - b[0], y = b[4] - b[1], z = b[5] - b[2];
    return 2.0f * (x * y + y * z + z * x);
}
int emitter_boxes(const float* root, float* out) {
    float bx[4][6];
    int n = 0;
    int32_t links[4];
    std::memcpy(links, root + 24, sizeof links);
    for (int k = 0; k < 4; ++k) {
        if (links[k] < 0) continue;
        for (int i = 0; i < 6; ++i) {
            if (!std::isfinite(root[6 * k + i])) return 0;
            bx[n][i] = root[6 * k + i];
        }
        ++n;
    }
    for (bool merged = true; merged && n > 1;) {
        merged = false;
        for (int a = 0; a < n && !merged; ++a)
            for (int b = a + 1; b < n && !merged; ++b) {
                float u[6];
                for (int i = 0; i < 3; ++i) {
                    u[i] = std::min(bx[a][i], bx[b][i]);
                    u[3 + i] = std::max(bx[a][3 + i], bx[b][3 + i]);
                }
                if (box_area(u) <= box_area(bx[a]) + box_area(bx[b])) {
                    std::memcpy(bx[a], u, sizeof u);
                    std::memcpy(bx[b], bx[n - 1], sizeof u);
                    --n;
                    merged = true;
                }
            }
    }
    for (int k = 0; k < n; ++k) std::memcpy(out + 6 * k, bx[k], sizeof bx[k]);
    return n;
}

// Uploads a finished HostTrees job and completes the scene (the stack bound).
tpt_status upload_host_trees(tpt_scene* s, HostTrees& j, uint32_t* wide_need) {
    if (j.st != TPT_OK) return fail(j.st, j.msg);
    s->lv_main.clear();
    s->lv_emit.clear();
    if (j.main_ok()) {
        HIP_OR_FAIL(hipMemcpyAsync(s->inner4.p, j.w4.data(), j.w4.size() * sizeof(float), hipMemcpyHostToDevice,
                                   s->stream));
        s->n4 = j.n4;
        *wide_need = (uint32_t)j.need;
        s->wide_tree = 1;
    }
    if (j.emit_ok()) {
        HIP_OR_FAIL(hipMemcpyAsync(s->inner4.p + 8 * (size_t)s->n4, j.e4.data(), j.e4.size() * sizeof(float),
                                   hipMemcpyHostToDevice, s->stream));
        s->emit_root = s->n4;
        s->n_emit4 = j.ne4;
        s->n_emit_box = emitter_boxes(j.e4.data(), s->emit_box);
        *wide_need = std::max(*wide_need, (uint32_t)j.eneed);
    }
    // a refit's launches (tpt_scene_refit), while the copies run: one level of a tree each.
    // Trees that are not level-ordered leave lv_main empty, and a refit rebuilds.
    try {
        if (j.main_ok() && tpt::wide_tree_levels(j.w4.data(), j.n4, 0, s->lv_main) < 1) s->lv_main.clear();
        if (j.emit_ok() && !s->lv_main.empty()) {
            if (tpt::wide_tree_levels(j.e4.data(), j.ne4, s->emit_root, s->lv_emit) < 1) s->lv_main.clear();
            for (int32_t& v : s->lv_emit) v += s->emit_root;
        }
    } catch (const std::bad_alloc&) {
        s->lv_main.clear();
    }
    HIP_OR_FAIL(hipStreamSynchronize(s->stream));   // (the host buffers are freed after this)
    return TPT_OK;
}

// Stack capacity: the binary DFS that pushes one sibling per level holds at
// most depth + 1 entries; the 4-wide ordered walk holds at most the tree's
// stack need (wide_bvh.cpp), 3 * ceil(depth / 2) for the LBVH's even-depth view.
tpt_status finish_stack(tpt_scene* s, uint32_t wide_need) {
    s->stack_depth = (int32_t)std::max<uint32_t>(std::max<uint32_t>(s->tree_depth + 2, wide_need), 2);
    if (s->stack_depth > 160) return fail(TPT_ERR_INVALID_ARG, "BVH deeper than the LDS stack supports");
    s->built = true;
    s->resident = true;
    return TPT_OK;
}

// The traversal-exactness inputs both scene_build and tpt_scene_refit derive from k_sliver_scan
// (trace.hip "Culling").  The culls' absolute position slack: 4 ulps of the largest world coordinate.
float cull_eps_of(double max_coord) {
    if (!(std::isfinite(max_coord) && max_coord > 0.0)) return 0.0f;
    int ex = 0;
    (void)std::frexp(max_coord, &ex);             // max_coord < 2^ex
    return (float)std::ldexp(4.0, ex - 24);       // 4 ulps of a float below 2^ex
}

// The sliver list and its groups from the flagged positions `sl` (reordered), the leaf boxes and
// the emitter flags by position; uploads them and sets n_sliver_groups.
tpt_status upload_slivers(tpt_scene* s, std::vector<int>& sl, const float* lbox, const uint32_t* lemit) {
    s->n_sliver_groups = 0;
    if (sl.empty()) return TPT_OK;
    // groups 1..: split the list at the median of the longest centroid axis
    // while a group holds more than 8 slivers and there are < 8 groups;
    // group 0 is the union of all (tested first by every ray)
    std::vector<std::pair<int, int>> grp{{0, (int)sl.size()}};
    auto cen = [&](int p, int k) { return lbox[6 * p + k] + lbox[6 * p + 3 + k]; };
    for (bool split = true; split && grp.size() < 8;) {
        split = false;
        size_t big = 0;
        for (size_t g = 1; g < grp.size(); ++g)
            if (grp[g].second - grp[g].first > grp[big].second - grp[big].first) big = g;
        const int b0 = grp[big].first, b1 = grp[big].second;
        if (b1 - b0 <= 8) break;
        float lo[3] = {kInfF, kInfF, kInfF}, hi[3] = {-kInfF, -kInfF, -kInfF};
        for (int i = b0; i < b1; ++i)
            for (int k = 0; k < 3; ++k) {
                lo[k] = std::min(lo[k], cen(sl[i], k));
                hi[k] = std::max(hi[k], cen(sl[i], k));
            }
        int ax = 0;
        for (int k = 1; k < 3; ++k)
            if (hi[k] - lo[k] > hi[ax] - lo[ax]) ax = k;
        const int mid = (b0 + b1) / 2;
        std::nth_element(sl.begin() + b0, sl.begin() + mid, sl.begin() + b1,
                         [&](int x, int y) { return cen(x, ax) < cen(y, ax); });
        grp[big] = {b0, mid};
        grp.push_back({mid, b1});
        split = true;
    }
    grp.insert(grp.begin(), {0, (int)sl.size()});   // group 0: the union
    std::vector<float4> gb(2 * grp.size());
    std::vector<float4> lst(2 * sl.size());   // exact leaf box, position | emissive << 30
    for (size_t i = 0; i < sl.size(); ++i) {
        const int32_t e = sl[i] | (lemit[sl[i]] ? (1 << 30) : 0);
        float fe;
        std::memcpy(&fe, &e, 4);
        const float* b = &lbox[6 * sl[i]];
        lst[2 * i] = make_float4(b[0], b[1], b[2], fe);
        lst[2 * i + 1] = make_float4(b[3], b[4], b[5], 0.0f);
    }
    for (size_t g = 0; g < grp.size(); ++g) {
        float lo[3] = {kInfF, kInfF, kInfF}, hi[3] = {-kInfF, -kInfF, -kInfF};
        for (int i = grp[g].first; i < grp[g].second; ++i)
            for (int k = 0; k < 3; ++k) {
                lo[k] = std::min(lo[k], lbox[6 * sl[i] + k]);
                hi[k] = std::max(hi[k], lbox[6 * sl[i] + 3 + k]);
            }
        int32_t first = grp[g].first, count = grp[g].second - grp[g].first;
        float ff, fc;
        std::memcpy(&ff, &first, 4);
        std::memcpy(&fc, &count, 4);
        gb[2 * g] = make_float4(lo[0], lo[1], lo[2], ff);
        gb[2 * g + 1] = make_float4(hi[0], hi[1], hi[2], fc);
    }
    HIP_OR_FAIL(s->sliver_groups.upload(gb.data(), gb.size(), s->stream));
    HIP_OR_FAIL(s->sliver_list.upload(lst.data(), lst.size(), s->stream));
    HIP_OR_FAIL(hipStreamSynchronize(s->stream));   // (gb and lst are freed below)
    s->n_sliver_groups = (int32_t)grp.size();
    return TPT_OK;
}

// The positions k_sliver_scan flagged and the largest coordinate's bits behind them (n flags,
// then the 8 bytes of coord_max), as both callers read them back
void read_sliver_scan(const uint8_t* lsliver, size_t n, std::vector<int>& sl, double* max_coord) {
    sl.clear();
    for (size_t p = 0; p < n; ++p)
        if (lsliver[p]) sl.push_back((int)p);
    unsigned long long mbits = 0;
    std::memcpy(&mbits, lsliver + n, sizeof mbits);
    std::memcpy(max_coord, &mbits, sizeof *max_coord);
}

// The scene's buffers as the build and refit kernels take them
void fill_build_buffers(tpt_scene* s, size_t sort_bytes, tpt::BuildBuffers& b) {
    b.n_faces = s->n_faces;
    b.n_vertices = s->n_vertices;
    b.n_objects = s->n_objects;
    b.n_materials = s->n_materials;
    b.indices = s->indices.p;
    b.vertices = s->vertices.p;
    b.normals = s->normals.p;
    b.lut = s->lut.p;
    b.vert_trans = s->vert_trans.p;
    b.normal_trans = s->normal_trans.p;
    b.mtl = s->mtl.p;
    b.wverts = s->wverts.p;
    b.wnorms = s->wnorms.p;
    b.keys = s->keys.p;
    b.keys_sorted = s->keys_sorted.p;
    b.fids = s->fids.p;
    b.fids_sorted = s->fids_sorted.p;
    b.leaf_box = s->leaf_box.p;
    b.children = s->children.p;
    b.parent = s->parent.p;
    b.node_box = s->node_box.p;
    b.flags = s->flags.p;
    b.max_depth = s->max_depth.p;
    b.sort_tmp = s->sort_tmp.p;
    b.sort_tmp_bytes = sort_bytes;
    b.inner = s->inner.p;
    b.inner4 = s->inner4.p;
    b.bfs_keys = s->bfs_keys.p;
    b.bfs_keys_sorted = s->bfs_keys_sorted.p;
    b.bfs_ids = s->bfs_ids.p;
    b.bfs_ids_sorted = s->bfs_ids_sorted.p;
    b.bfs_newid = s->bfs_newid.p;
    b.emit = s->emit.p;
    b.tri = s->tri.p;
    b.shade = s->shade.p;
    b.nodes36 = s->nodes36.p;
}

tpt_status scene_build(tpt_scene* s, bool async) {
    if (!s) return fail(TPT_ERR_INVALID_ARG, "null scene");
    if (s->trees) s->trees->join();   // a previous asynchronous build still running: its trees are superseded
    s->pending = false;
    s->built = false;
    s->resident = false;           // (finish_stack sets it again)
    s->cost_built_valid = false;
    DeviceGuard g(s->device);
    const size_t n = (size_t)s->n_faces, nn = 2 * n - 1, nv = (size_t)s->n_vertices;
    size_t sort_bytes = 0;
    HIP_OR_FAIL(tpt::build_sort_tmp_bytes((int32_t)n, &sort_bytes));
    HIP_OR_FAIL(s->wverts.alloc(3 * nv));
    HIP_OR_FAIL(s->wnorms.alloc(3 * nv));
    HIP_OR_FAIL(hipMemsetAsync(s->wverts.p, 0, 3 * nv * sizeof(float), s->stream));
    HIP_OR_FAIL(hipMemsetAsync(s->wnorms.p, 0, 3 * nv * sizeof(float), s->stream));
    HIP_OR_FAIL(s->keys.alloc(n));
    HIP_OR_FAIL(s->keys_sorted.alloc(n));
    HIP_OR_FAIL(s->fids.alloc(n));
    HIP_OR_FAIL(s->fids_sorted.alloc(n));
    HIP_OR_FAIL(s->leaf_box.alloc(6 * n));
    HIP_OR_FAIL(s->children.alloc(std::max<size_t>(n - 1, 1)));
    HIP_OR_FAIL(s->parent.alloc(nn));
    HIP_OR_FAIL(s->node_box.alloc(6 * nn));
    HIP_OR_FAIL(s->flags.alloc(nn));
    HIP_OR_FAIL(s->max_depth.alloc(3));
    HIP_OR_FAIL(s->bfs_keys.alloc(std::max<size_t>(n - 1, 1)));
    HIP_OR_FAIL(s->bfs_keys_sorted.alloc(std::max<size_t>(n - 1, 1)));
    HIP_OR_FAIL(s->bfs_ids.alloc(std::max<size_t>(n - 1, 1)));
    HIP_OR_FAIL(s->bfs_ids_sorted.alloc(std::max<size_t>(n - 1, 1)));
    HIP_OR_FAIL(s->bfs_newid.alloc(std::max<size_t>(n - 1, 1)));
    HIP_OR_FAIL(s->emit.alloc(nn));
    HIP_OR_FAIL(s->sort_tmp.alloc(std::max<size_t>(sort_bytes, 16)));
    HIP_OR_FAIL(s->inner.alloc(4 * std::max<size_t>(n - 1, 1)));
    HIP_OR_FAIL(s->inner4.alloc(8 * std::max<size_t>(n - 1, 1)));
    HIP_OR_FAIL(s->tri.alloc(tpt::tri_float4s(n)));
    HIP_OR_FAIL(s->shade.alloc(3 * n));
    HIP_OR_FAIL(s->nodes36.alloc(36 * nn));
    HIP_OR_FAIL(hipMemsetAsync(s->parent.p, 0, nn * sizeof(uint32_t), s->stream));
    PhaseClock clk(std::getenv("TPT_BUILD_TIMING") != nullptr);

    tpt::BuildBuffers b{};
    fill_build_buffers(s, sort_bytes, b);
    {
        const hipError_t be = tpt::launch_build(b, s->stream);
        if (be != hipSuccess && b.out_max_depth >= tpt::kMaxLbvhDepth)
            return fail(TPT_ERR_INVALID_ARG,
                        "LBVH topology invalid: duplicate Morton keys made a node's parent chain miss the root "
                        "(computeNodeRange, bvh.cu:150-217, has no tie-break; the reference would not terminate)");
        HIP_OR_FAIL(be);
    }
    s->tree_depth = b.out_max_depth;
    s->boxes_finite = (int32_t)b.out_boxes_finite;
    s->n4 = (int32_t)b.out_n4;
    {   // the root's emitter flag: does any triangle emit (a probe can only add emission)
        uint32_t root_emit = 1;
        HIP_OR_FAIL(hipMemcpyAsync(&root_emit, s->emit.p, sizeof root_emit, hipMemcpyDeviceToHost, s->stream));
        HIP_OR_FAIL(hipStreamSynchronize(s->stream));
        s->any_emitter = root_emit != 0 ? 1 : 0;
    }
    clk.mark("lbvh");
    const uint32_t td = b.out_max_depth;
    uint32_t wide_need = 3 * ((td + 1) / 2) + 1;
    s->wide_tree = 0;
    s->emit_root = -1;
    s->n_emit4 = 0;
    s->n_emit_box = 0;
    s->slivers = 0;
    s->n_sliver_groups = 0;
    s->cull_eps = 0.0f;
    if (n > 1 && s->boxes_finite) {
        // Culling exactness (trace.hip "Culling"): sliver triangles -- sin of the
        // angle at v0 between the edges rayHitTriangle uses below 1e-3 -- give
        // an arbitrary t, so they are listed (in up to 4 groups with union
        // boxes) and re-tested after every culled traversal; the culls'
        // absolute position slack is 4 ulps of the largest world coordinate (a
        // hit point, the next ray's origin, is rounded to its ulp; an edge hit
        // accepted by barycentric rounding lies a few ulps outside its triangle).
        // Both come from k_sliver_scan; the leaf boxes and emitter flags (for
        // the host trees) come back with them into pinned staging.
        HIP_OR_FAIL(s->sliver_flags.alloc(n));
        HIP_OR_FAIL(s->coord_max.alloc(1));
        HIP_OR_FAIL(hipMemsetAsync(s->coord_max.p, 0, sizeof(unsigned long long), s->stream));
        HIP_OR_FAIL(tpt::launch_sliver_scan(s->tri.p, (int32_t)n, s->sliver_flags.p, s->coord_max.p, s->stream));
        HIP_OR_FAIL(s->h_lbox.alloc(6 * n));
        HIP_OR_FAIL(s->h_lemit.alloc(n));
        HIP_OR_FAIL(s->h_sliver.alloc(n + 8));
        float* const lbox = s->h_lbox.p;
        uint32_t* const lemit = s->h_lemit.p;
        uint8_t* const lsliver = s->h_sliver.p;
        HIP_OR_FAIL(hipMemcpyAsync(lbox, s->node_box.p + 6 * (n - 1), 6 * n * sizeof(float), hipMemcpyDeviceToHost,
                                   s->stream));
        HIP_OR_FAIL(hipMemcpyAsync(lemit, s->emit.p + (n - 1), n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        HIP_OR_FAIL(hipMemcpyAsync(lsliver, s->sliver_flags.p, n, hipMemcpyDeviceToHost, s->stream));
        HIP_OR_FAIL(hipMemcpyAsync(lsliver + n, s->coord_max.p, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   s->stream));
        HIP_OR_FAIL(hipStreamSynchronize(s->stream));
        clk.mark("readback");
        std::vector<int> sl;
        double max_coord = 0.0;
        read_sliver_scan(lsliver, n, sl, &max_coord);
        s->slivers = (int32_t)sl.size();
        s->cull_eps = cull_eps_of(max_coord);
        {
            const tpt_status ss = upload_slivers(s, sl, lbox, lemit);
            if (ss != TPT_OK) return ss;
        }
        clk.mark("slivers");
        if (!s->trees) {
            try {
                s->trees = std::make_unique<HostTrees>();
            } catch (const std::bad_alloc&) {
                return fail(TPT_ERR_OOM, "traversal tree build: host allocation failed");
            }
        }
        HostTrees& j = *s->trees;
        j.reset_results();
        j.n = n;
        j.lbox = lbox;     // the scene's pinned staging: the next build joins this job first
        j.lemit = lemit;
        j.prm.threads = s->build_threads;
#ifdef TPT_WIDE_SWEEP
        j.prm.sweep_max = TPT_WIDE_SWEEP;   // A/B builds: exact-sweep threshold
#endif
        j.lbvh_n4 = s->n4;
        j.timing = clk.on;
        if (async) {
            s->pending_need = wide_need;
            HostTrees* jp = &j;
            try {
                j.th = std::thread([jp] { build_host_trees(*jp); });
                s->pending = true;
                s->built = true;   // (finish_pending completes it)
                return TPT_OK;
            } catch (const std::exception&) {   // no thread (system_error, bad_alloc): build it here
            }
        }
        build_host_trees(j);
        const tpt_status st = upload_host_trees(s, j, &wide_need);
        if (st != TPT_OK) return st;
        clk.mark("upload");
    }
    return finish_stack(s, wide_need);
}

// tpt_refit_stats.cost of the resident main tree into cost_out[2 * slot], [2 * slot + 1]
tpt_status enqueue_cost(tpt_scene* s, int slot, int32_t* launches) {
    HIP_OR_FAIL(s->cost_terms.alloc((size_t)s->n4));
    HIP_OR_FAIL(s->cost_out.alloc(4));
    HIP_OR_FAIL(s->h_cost.alloc(4));
    HIP_OR_FAIL(tpt::launch_wide_cost(s->inner4.p, s->n4, s->cost_terms.p, s->cost_out.p + 2 * slot, launches, s->stream));
    HIP_OR_FAIL(hipMemcpyAsync(s->h_cost.p + 2 * slot, s->cost_out.p + 2 * slot, 2 * sizeof(double),
                               hipMemcpyDeviceToHost, s->stream));
    return TPT_OK;
}
double cost_ratio(const double* c) { return c[1] > 0.0 ? c[0] / c[1] : 0.0; }

// The end of every tpt_scene_refit: the stats, with the device time between the two events
tpt_status refit_done(tpt_scene* s, tpt_refit_stats* st, tpt_refit_stats& r) {
    HIP_OR_FAIL(hipEventRecord(s->ev[1], s->stream));
    HIP_OR_FAIL(hipEventSynchronize(s->ev[1]));
    float ms = 0.0f;
    HIP_OR_FAIL(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    r.ms = ms;
    r.slivers = s->slivers;
    r.cull_eps = s->cull_eps;
    if (st) *st = r;
    return TPT_OK;
}

// The fallback: a full build, and (with an SAH tree) its cost, which is then the built one
tpt_status refit_rebuild(tpt_scene* s, tpt_refit_stats* st, tpt_refit_stats& r) {
    r.rebuilt = 1;
    const tpt_status bs = scene_build(s, false);
    if (bs != TPT_OK) return bs;
    if (s->wide_tree && s->n4 > 0) {
        const tpt_status cs = enqueue_cost(s, 0, &r.launches);
        if (cs != TPT_OK) return cs;
        HIP_OR_FAIL(hipStreamSynchronize(s->stream));
        s->cost_built = cost_ratio(s->h_cost.p);
        s->cost_built_valid = true;
        r.cost = r.cost_built = s->cost_built;
    }
    return refit_done(s, st, r);
}

tpt_status scene_refit(tpt_scene* s, tpt_refit_stats* st) {
    if (!s) return fail(TPT_ERR_INVALID_ARG, "null scene");
    tpt_refit_stats r{};
    {   // a pending build that no tpt_scene_set_* superseded is finished first
        const tpt_status ps = finish_pending(s);
        if (ps != TPT_OK) return ps;
    }
    DeviceGuard g(s->device);
    s->acc_valid = false;   // a progressive accumulation's sums belong to the scene as it was
    HIP_OR_FAIL(hipEventRecord(s->ev[0], s->stream));
    const size_t n = (size_t)s->n_faces, nv = (size_t)s->n_vertices;
    if (!s->resident || !s->wide_tree || n < 2 || s->lv_main.empty() || s->n4 <= 0) return refit_rebuild(s, st, r);
    s->built = false;
    if (!s->cost_built_valid) {   // the trees are still the build's: their cost, before a box changes
        const tpt_status cs = enqueue_cost(s, 0, &r.launches);
        if (cs != TPT_OK) return cs;
    }
    tpt::BuildBuffers b{};
    fill_build_buffers(s, 0, b);
    HIP_OR_FAIL(hipMemsetAsync(s->wverts.p, 0, 3 * nv * sizeof(float), s->stream));
    HIP_OR_FAIL(hipMemsetAsync(s->wnorms.p, 0, 3 * nv * sizeof(float), s->stream));
    tpt::RefitPlan plan{};
    plan.tree_depth = s->tree_depth;
    plan.lv_main = s->lv_main.data();
    plan.n_lv_main = (int32_t)s->lv_main.size() - 1;
    plan.lv_emit = s->lv_emit.data();
    plan.n_lv_emit = s->lv_emit.empty() ? 0 : (int32_t)s->lv_emit.size() - 1;
    HIP_OR_FAIL(tpt::launch_refit(b, plan, &r.launches, s->stream));
    HIP_OR_FAIL(hipMemsetAsync(s->coord_max.p, 0, sizeof(unsigned long long), s->stream));
    HIP_OR_FAIL(tpt::launch_sliver_scan(s->tri.p, (int32_t)n, s->sliver_flags.p, s->coord_max.p, s->stream));
    ++r.launches;
    {
        const tpt_status cs = enqueue_cost(s, 1, &r.launches);
        if (cs != TPT_OK) return cs;
    }
    // the small read-backs, then the one synchronisation: the non-finite word, the sliver flags
    // with the largest coordinate, the emissive tree's root node
    HIP_OR_FAIL(s->h_nonfinite.alloc(1));
    HIP_OR_FAIL(s->h_eroot.alloc(32));
    uint8_t* const lsliver = s->h_sliver.p;   // (n + 8 bytes since the build)
    HIP_OR_FAIL(hipMemcpyAsync(s->h_nonfinite.p, s->max_depth.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_OR_FAIL(hipMemcpyAsync(lsliver, s->sliver_flags.p, n, hipMemcpyDeviceToHost, s->stream));
    HIP_OR_FAIL(hipMemcpyAsync(lsliver + n, s->coord_max.p, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               s->stream));
    if (s->emit_root >= 0)
        HIP_OR_FAIL(hipMemcpyAsync(s->h_eroot.p, s->inner4.p + 8 * (size_t)s->emit_root, 32 * sizeof(float),
                                   hipMemcpyDeviceToHost, s->stream));
    HIP_OR_FAIL(hipStreamSynchronize(s->stream));
    if (!s->cost_built_valid) {
        s->cost_built = cost_ratio(s->h_cost.p);
        s->cost_built_valid = true;
    }
    if (s->h_nonfinite.p[0] != 0) return refit_rebuild(s, st, r);   // a non-finite vertex or box: what a build makes of it
    s->boxes_finite = 1;
    std::vector<int> sl;
    double max_coord = 0.0;
    try {
        read_sliver_scan(lsliver, n, sl, &max_coord);
    } catch (const std::bad_alloc&) {
        return fail(TPT_ERR_OOM, "refit: host allocation failed");
    }
    s->slivers = (int32_t)sl.size();
    s->cull_eps = cull_eps_of(max_coord);
    s->n_sliver_groups = 0;
    if (!sl.empty()) {
        // slivers are rare: only then do the leaf boxes come back (the emitter flags by position
        // are the build's, still in the pinned staging)
        HIP_OR_FAIL(hipMemcpyAsync(s->h_lbox.p, s->node_box.p + 6 * (n - 1), 6 * n * sizeof(float),
                                   hipMemcpyDeviceToHost, s->stream));
        HIP_OR_FAIL(hipStreamSynchronize(s->stream));
        const tpt_status ss = upload_slivers(s, sl, s->h_lbox.p, s->h_lemit.p);
        if (ss != TPT_OK) return ss;
    }
    if (s->emit_root >= 0) s->n_emit_box = emitter_boxes(s->h_eroot.p, s->emit_box);
    r.cost = cost_ratio(s->h_cost.p + 2);
    r.cost_built = s->cost_built;
    s->built = true;
    return refit_done(s, st, r);
}

}  // namespace

tpt_status tpt::host::finish_pending(tpt_scene* s, double* wait_ms) {
    if (!s->pending) return TPT_OK;
    const auto t0 = std::chrono::steady_clock::now();
    HostTrees& j = *s->trees;
    j.join();
    s->pending = false;
    if (wait_ms) *wait_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    DeviceGuard g(s->device);
    uint32_t wide_need = s->pending_need;
    tpt_status st = upload_host_trees(s, j, &wide_need);
    if (st == TPT_OK) st = finish_stack(s, wide_need);
    if (st != TPT_OK) s->built = false;
    return st;
}

extern "C" {

tpt_status tpt_scene_create(const tpt_scene_desc* d_in, int device, tpt_scene** out) {
    if (!d_in || !out) return fail(TPT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (d_in->n_faces == 0 || !d_in->indices || !d_in->vertices || !d_in->normals || d_in->n_vertices == 0)
        return fail(TPT_ERR_INVALID_ARG, "scene needs faces, vertices and normals");
    if (d_in->n_objects == 0 || !d_in->lut || !d_in->vert_trans || !d_in->normal_trans)
        return fail(TPT_ERR_INVALID_ARG, "scene needs at least one object (LUT + transforms)");
    if (d_in->n_lights > (uint32_t)tpt::kMaxLights) return fail(TPT_ERR_INVALID_ARG, "too many delta lights (max 16)");
    if (d_in->n_lights > 0 && !d_in->lights) return fail(TPT_ERR_INVALID_ARG, "null light array");
    if (d_in->n_faces > (1u << 30)) return fail(TPT_ERR_INVALID_ARG, "too many faces");
    if (d_in->flags & ~(uint32_t)TPT_DESC_DELTALIGHT_LAYOUT) return fail(TPT_ERR_INVALID_ARG, "unknown desc flags");
    int ndev = tpt_device_count();
    if (ndev <= 0) return fail(TPT_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(TPT_ERR_INVALID_ARG, "bad device index");

    DeviceGuard g(device);
    // Arrays may live in device memory (DeviceScene's thrust buffers, the
    // `trace` kernel's arguments): the small ones and the indices (validated
    // here) are read back; vertices and normals are copied device to device.
    tpt_scene_desc dh = *d_in;
    const tpt_scene_desc* d = &dh;
    std::vector<uint32_t> t_idx;
    std::vector<tpt_interval> t_lut;
    std::vector<float> t_vt, t_nt;
    std::vector<tpt_material> t_mtl;
    std::vector<tpt_light> t_lights;
    hipError_t herr = hipSuccess;
    dh.indices = host_view(d_in->indices, 3 * (size_t)d_in->n_faces, t_idx, &herr);
    dh.lut = host_view(d_in->lut, d_in->n_objects, t_lut, &herr);
    dh.vert_trans = host_view(d_in->vert_trans, 16 * (size_t)d_in->n_objects, t_vt, &herr);
    dh.normal_trans = host_view(d_in->normal_trans, 16 * (size_t)d_in->n_objects, t_nt, &herr);
    dh.materials = host_view(d_in->materials, d_in->n_materials, t_mtl, &herr);
    dh.lights = host_view(d_in->lights, d_in->n_lights, t_lights, &herr);
    if (herr != hipSuccess) return fail(TPT_ERR_HIP, std::string("scene desc readback: ") + hipGetErrorString(herr));
    // Device vertices / normals are copied device to device on this scene's
    // stream, so they must live on `device` itself (another GPU's buffers would
    // need peer access): a buffer of another device is rejected.
    int v_owner = -1, n_owner = -1;
    const bool verts_dev = is_device_ptr(d_in->vertices, &v_owner), norms_dev = is_device_ptr(d_in->normals, &n_owner);
    if ((v_owner >= 0 && v_owner != device) || (n_owner >= 0 && n_owner != device))
        return fail(TPT_ERR_INVALID_ARG, "device vertex/normal buffers must live on the scene's device");

    for (uint64_t i = 0; i < 3ull * d->n_faces; ++i)
        if (d->indices[i] >= d->n_vertices) return fail(TPT_ERR_INVALID_ARG, "vertex index out of range");
    if (d->lut[0].begin != 0) return fail(TPT_ERR_INVALID_ARG, "first object must begin at face 0");

    tpt_scene* s = new (std::nothrow) tpt_scene();
    if (!s) return fail(TPT_ERR_OOM, "host allocation failed");
    s->device = device;
    auto cleanup = [&](tpt_status st) {
        delete s;
        return st;
    };
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    for (int i = 0; e == hipSuccess && i < 5; ++i) e = hipEventCreate(&s->ev[i]);
    if (e != hipSuccess) return cleanup(fail(TPT_ERR_HIP, std::string("stream/event: ") + hipGetErrorString(e)));
    {
        // the launch rules that key on the chip's resident lanes (launch_plan.cpp:
        // four lanes per pixel, drained launches) take them from the device
        hipDeviceProp_t prop{};
        e = hipGetDeviceProperties(&prop, device);
        if (e != hipSuccess) return cleanup(fail(TPT_ERR_HIP, std::string("device properties: ") + hipGetErrorString(e)));
        s->n_cu = prop.multiProcessorCount;
        s->resident_lanes = (uint64_t)std::max(s->n_cu, 1) * 4u * (uint64_t)tpt::trace_waves_per_simd() * 64u;
    }

    s->n_faces = (int32_t)d->n_faces;
    s->n_vertices = (int32_t)d->n_vertices;
    s->n_objects = (int32_t)d->n_objects;
    s->n_materials = (int32_t)d->n_materials;
    s->n_lights = (int32_t)d->n_lights;

    std::vector<int2> lut(d->n_objects);
    for (uint32_t i = 0; i < d->n_objects; ++i) lut[i] = make_int2(d->lut[i].begin, d->lut[i].mtl);
    // materials + one Material() slot for meshes without a material (App. A.9)
    std::vector<float4> mtl(2 * ((size_t)d->n_materials + 1));
    s->unwind_prune = 1;   // k_trace's pruned unwind needs every colour of the table, the Material() slot included
    for (uint32_t i = 0; i <= d->n_materials; ++i) {
        tpt_material m = (i < d->n_materials && d->materials) ? d->materials[i] : tpt::default_material();
        for (int c = 0; c < 3; ++c)
            if (!tpt::prune_color_ok(m.base_color[c])) s->unwind_prune = 0;
        mtl[2 * i] = make_float4(m.base_color[0], m.base_color[1], m.base_color[2], m.emission_factor);
        mtl[2 * i + 1] = make_float4(m.eta, m.metallic, 0.0f, 0.0f);
    }
    const bool union_layout = (d->flags & TPT_DESC_DELTALIGHT_LAYOUT) != 0;
    std::vector<tpt::DevLight> lights(d->n_lights);
    for (uint32_t i = 0; i < d->n_lights; ++i) {
        const tpt_light& L = d->lights[i];
        if (L.type < 0 || L.type > 2) return cleanup(fail(TPT_ERR_INVALID_ARG, "unknown delta light type"));
        tpt::DevLight& o = lights[i];
        o.type = L.type;
        std::memcpy(o.color, L.color, sizeof o.color);
        o.intensity = L.intensity;
        if (union_layout) {
            // DeltaLight (delta_light.h:96-130): the union's members share their
            // first bytes -- color, intensity, then PointLight::pos /
            // DirectionalLight::direction / SpotLight::pos; only a spot light has
            // the direction and cone fields behind them.  Bytes a light type does
            // not own are not read.
            std::memset(o.pos, 0, sizeof o.pos);
            std::memset(o.dir, 0, sizeof o.dir);
            o.cos_outer = 0.0f;
            o.inv_cos_cone_diff = 0.0f;
            if (L.type == 1) {
                std::memcpy(o.dir, L.pos, sizeof o.dir);
            } else {
                std::memcpy(o.pos, L.pos, sizeof o.pos);
                if (L.type == 2) {
                    std::memcpy(o.dir, L.direction, sizeof o.dir);
                    o.cos_outer = L.cos_outer;
                    o.inv_cos_cone_diff = L.inv_cos_cone_diff;
                }
            }
        } else {
            std::memcpy(o.pos, L.pos, sizeof o.pos);
            std::memcpy(o.dir, L.direction, sizeof o.dir);
            o.cos_outer = L.cos_outer;
            o.inv_cos_cone_diff = L.inv_cos_cone_diff;
        }
    }
    const auto& jumps = host_jumps();
    hipStream_t st = s->stream;
    auto copy_in = [&](DevBuf<float>& dst, const float* src, size_t count, bool dev) {
        if (!dev) return dst.upload(src, count, st);
        hipError_t e2 = dst.alloc(count);
        if (e2 == hipSuccess) e2 = hipMemcpyAsync(dst.p, src, count * sizeof(float), hipMemcpyDeviceToDevice, st);
        return e2;
    };
    e = s->indices.upload(d->indices, 3 * (size_t)d->n_faces, st);
    if (e == hipSuccess) e = copy_in(s->vertices, d_in->vertices, 3 * (size_t)d->n_vertices, verts_dev);
    if (e == hipSuccess) e = copy_in(s->normals, d_in->normals, 3 * (size_t)d->n_vertices, norms_dev);
    if (e == hipSuccess) e = s->lut.upload(lut.data(), lut.size(), st);
    if (e == hipSuccess) e = s->vert_trans.upload(d->vert_trans, 16 * (size_t)d->n_objects, st);
    if (e == hipSuccess) e = s->normal_trans.upload(d->normal_trans, 16 * (size_t)d->n_objects, st);
    if (e == hipSuccess) e = s->mtl.upload(mtl.data(), mtl.size(), st);
    if (e == hipSuccess && !lights.empty()) e = s->lights.upload(lights.data(), lights.size(), st);
    if (e == hipSuccess) e = s->jumps.upload(jumps.data(), jumps.size(), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess)
        return cleanup(fail(e == hipErrorOutOfMemory ? TPT_ERR_OOM : TPT_ERR_HIP,
                            std::string("scene upload: ") + hipGetErrorString(e)));
    s->h_vert_trans.assign(d->vert_trans, d->vert_trans + 16 * (size_t)d->n_objects);
    s->h_lut_begin.resize(d->n_objects);
    for (uint32_t i = 0; i < d->n_objects; ++i) s->h_lut_begin[i] = d->lut[i].begin;
    *out = s;
    return TPT_OK;
}

// New local-to-world matrices for some objects.  The vertices stay on the device: the next
// build transforms them again (scene_build starts from vert_trans / normal_trans every time).
tpt_status tpt_scene_set_transforms(tpt_scene* s, uint32_t first, uint32_t n, const float* vert_trans,
                                    const float* normal_trans) {
    if (!s) return fail(TPT_ERR_INVALID_ARG, "null scene");
    if (!vert_trans) return fail(TPT_ERR_INVALID_ARG, "null vert_trans");
    if (n == 0) return fail(TPT_ERR_INVALID_ARG, "n_objects must be > 0");
    if ((uint64_t)first + (uint64_t)n > (uint64_t)s->n_objects)
        return fail(TPT_ERR_INVALID_ARG, "object range past the scene's object count");
    std::vector<float> nt;
    if (!normal_trans) {
        nt.resize(16 * (size_t)n);
        for (uint32_t i = 0; i < n; ++i) tpt::normal_to_world16(vert_trans + 16 * (size_t)i, nt.data() + 16 * (size_t)i);
        normal_trans = nt.data();
    }
    if (s->trees) s->trees->join();   // a pending asynchronous build is superseded, as by the next build
    s->pending = false;
    s->built = false;
    DeviceGuard g(s->device);
    const size_t off = 16 * (size_t)first, bytes = 16 * (size_t)n * sizeof(float);
    HIP_OR_FAIL(hipMemcpyAsync(s->vert_trans.p + off, vert_trans, bytes, hipMemcpyHostToDevice, s->stream));
    HIP_OR_FAIL(hipMemcpyAsync(s->normal_trans.p + off, normal_trans, bytes, hipMemcpyHostToDevice, s->stream));
    HIP_OR_FAIL(hipStreamSynchronize(s->stream));   // (the caller's matrices and nt are only read during the call)
    std::memcpy(s->h_vert_trans.data() + off, vert_trans, bytes);
    return TPT_OK;
}

// New object-space positions (and normals) for some vertices.  Topology, materials and matrices
// stay: the next build transforms the vertices again and rebuilds the BVH from them.
tpt_status tpt_scene_set_vertices(tpt_scene* s, uint32_t first, uint32_t n, const float* vertices,
                                  const float* normals) {
    if (!s) return fail(TPT_ERR_INVALID_ARG, "null scene");
    if (!vertices) return fail(TPT_ERR_INVALID_ARG, "null vertices");
    if (n == 0) return fail(TPT_ERR_INVALID_ARG, "n_vertices must be > 0");
    if ((uint64_t)first + (uint64_t)n > (uint64_t)s->n_vertices)
        return fail(TPT_ERR_INVALID_ARG, "vertex range past the scene's vertex count");
    DeviceGuard g(s->device);
    // each pointer host or device memory, as tpt_scene_create takes them; a device buffer is
    // copied device to device on the scene's stream, so it must live on the scene's device
    int v_owner = -1, n_owner = -1;
    const bool verts_dev = is_device_ptr(vertices, &v_owner), norms_dev = is_device_ptr(normals, &n_owner);
    if ((v_owner >= 0 && v_owner != s->device) || (n_owner >= 0 && n_owner != s->device))
        return fail(TPT_ERR_INVALID_ARG, "device vertex/normal buffers must live on the scene's device");
    if (s->trees) s->trees->join();   // a pending asynchronous build is superseded, as by the next build
    s->pending = false;
    s->built = false;
    s->acc_valid = false;             // a progressive accumulation's sums belong to the scene as it was
    const size_t off = 3 * (size_t)first, bytes = 3 * (size_t)n * sizeof(float);
    HIP_OR_FAIL(hipMemcpyAsync(s->vertices.p + off, vertices, bytes,
                               verts_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
    if (normals)
        HIP_OR_FAIL(hipMemcpyAsync(s->normals.p + off, normals, bytes,
                                   norms_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
    HIP_OR_FAIL(hipStreamSynchronize(s->stream));   // (the caller's arrays are only read during the call)
    return TPT_OK;
}

tpt_status tpt_scene_set_build_threads(tpt_scene* s, int32_t threads) {
    if (!s) return fail(TPT_ERR_INVALID_ARG, "null scene");
    s->build_threads = threads;
    return TPT_OK;
}

tpt_status tpt_scene_build(tpt_scene* s) { return scene_build(s, false); }

tpt_status tpt_scene_build_async(tpt_scene* s) { return scene_build(s, true); }

tpt_status tpt_scene_refit(tpt_scene* s, tpt_refit_stats* stats) { return scene_refit(s, stats); }

tpt_status tpt_scene_read_wide(tpt_scene* s, float* nodes, int32_t cap, int32_t* n_main, int32_t* n_emit) {
    if (!s || !s->built) return fail(TPT_ERR_INVALID_ARG, "scene not built");
    {
        const tpt_status bs = finish_pending(s);
        if (bs != TPT_OK) return bs;
    }
    // (without the SAH tree inner4 holds the LBVH's even-depth view: n4 nodes, no emissive tree)
    const int32_t nm = s->n4;
    const int32_t ne = s->emit_root >= 0 ? s->n_emit4 : 0;
    if (n_main) *n_main = nm;
    if (n_emit) *n_emit = ne;
    if (nodes && cap >= nm + ne && nm + ne > 0) {
        DeviceGuard g(s->device);
        HIP_OR_FAIL(hipStreamSynchronize(s->stream));
        HIP_OR_FAIL(hipMemcpy(nodes, s->inner4.p, 32 * sizeof(float) * (size_t)(nm + ne), hipMemcpyDeviceToHost));
    }
    return TPT_OK;
}

void tpt_scene_destroy(tpt_scene* s) { delete s; }

tpt_status tpt_env_create(const uint8_t* rgba, int32_t w, int32_t h, int device, tpt_env** out) {
    if (!rgba || !out || w <= 0 || h <= 0) return fail(TPT_ERR_INVALID_ARG, "bad env arguments");
    *out = nullptr;
    int ndev = tpt_device_count();
    if (ndev <= 0) return fail(TPT_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(TPT_ERR_INVALID_ARG, "bad device index");
    DeviceGuard g(device);
    tpt_env* env = new (std::nothrow) tpt_env();
    if (!env) return fail(TPT_ERR_OOM, "host allocation failed");
    env->device = device;
    env->w = w;
    env->h = h;
    hipError_t e = env->texels.alloc((size_t)w * (size_t)h);
    if (e == hipSuccess) e = hipMemcpy(env->texels.p, rgba, (size_t)w * h * 4, hipMemcpyHostToDevice);
    std::vector<float> icond, irow, imarg;
    env->is_b = env_is_block(w, h);
    env->is_bw = (w + env->is_b - 1) / env->is_b;
    env->is_bh = (h + env->is_b - 1) / env->is_b;
    const int bw = env->is_bw, bh = env->is_bh;
    build_env_is(rgba, w, h, env->is_b, icond, irow, imarg, env->is_total);
    if (e == hipSuccess) e = env->is_cond.upload(icond.data(), icond.size(), nullptr);
    if (e == hipSuccess) e = env->is_row.upload(irow.data(), irow.size(), nullptr);
    if (e == hipSuccess) e = env->is_marg.upload(imarg.data(), imarg.size(), nullptr);
    {   // guide tables: block rows at the block-row count, columns at a quarter of a block row
        env->is_kr = pow2_at_least(bh);
        env->is_kc = pow2_at_least(std::max(1, bw / 4));
        std::vector<int32_t> gr((size_t)env->is_kr + 1), gc((size_t)bh * (env->is_kc + 1));
        build_guide(imarg.data(), bh, env->is_total, env->is_kr, gr.data());
        for (int by = 0; by < bh; ++by)
            build_guide(icond.data() + (size_t)by * bw, bw, irow[by], env->is_kc,
                        gc.data() + (size_t)by * (env->is_kc + 1));
        if (e == hipSuccess) e = env->is_guide_r.upload(gr.data(), gr.size(), nullptr);
        if (e == hipSuccess) e = env->is_guide_c.upload(gc.data(), gc.size(), nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        delete env;
        return fail(TPT_ERR_HIP, std::string("env upload: ") + hipGetErrorString(e));
    }
    *out = env;
    return TPT_OK;
}

void tpt_env_destroy(tpt_env* env) {
    if (!env) return;
    DeviceGuard g(env->device);
    delete env;
}

tpt_status tpt_env_load(const char* path, int device, tpt_env** out) {
    if (!path || !out) return fail(TPT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    uint8_t* px = nullptr;
    int32_t w = 0, h = 0;
    const tpt_status st = tpt_image_load(path, &px, &w, &h);
    if (st != TPT_OK) return st;
    const tpt_status st2 = tpt_env_create(px, w, h, device, out);
    tpt_image_free(px);
    return st2;
}

}  // extern "C"
