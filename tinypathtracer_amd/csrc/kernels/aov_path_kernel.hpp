// aov_path_kernel.hpp -- the text of k_aov_path, included by post.hip once as it is and once
// with TPT_AOV_PATH_POINTS as k_aov_path_points.  No include guard: it is meant to be read twice.

// k_aov continued through perfect mirrors (tpt_render_aov_path; DESIGN.md section 5
// "Post-pass" holds the definition the tests pin).  k_aov's lanes, tiles and LDS stack.  A
// lane traces, runs the hit prelude, and where the hit is a mirror below the cap reflects and
// goes round again from the hit point, as k_trace starts an extension ray: the origin advanced
// to o + t d, reflect_dir about the shading normal, the grazing rule with the face it leaves;
// rayHitTriangle's t > kDelta keeps the ray off that face, there is no offset.  A finished
// lane waits for its wave; the wave leaves when no lane continues, so a wave that meets no
// mirror does k_aov's one traversal.  Lanes outside the frame stay to the end (they never
// trace): the statistics are taken by the whole wave.
//
// TPT_AOV_PATH_POINTS (k_aov_path_points; tpt_render_aov_path_points): the lane also keeps
// where its path ended -- the terminal hit point, formed as the advance forms an origin, or
// the last ray's direction where the path leaves the scene -- and writes it as three floats.
#if TPT_AOV_PATH_POINTS
__global__ __launch_bounds__(256) void k_aov_path_points(TraceArgs a, AovArgs o, AovPathArgs p, float* points) {
#else
__global__ __launch_bounds__(256) void k_aov_path(TraceArgs a, AovArgs o, AovPathArgs p) {
#endif
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x;
    const int2 xy = tile_wave_xy(tid);
    const int x = xy.x, y = xy.y;
    const bool inside = x < a.width && y < a.height;   // (no barrier below)
    V3 ro, rd;
    centre_ray(a, x, y, ro, rd);
    Trav r;
    LaneStack<int> stk;
    stk.lds = (TPT_LDS int*)lds + tid;
    stk.nlds = kAovLdsSlots;
    V3 alb = v3(1.0f, 1.0f, 1.0f), nrm = v3(0.0f, 0.0f, 0.0f);   // the product of the base colours so far
    float depth = 0.0f;                                          // the distance travelled so far
    int fid = -1, mtl = -1, k = 0;
    bool tg = false;   // the camera: no surface
    bool live = inside;
#if TPT_AOV_PATH_POINTS
    V3 end = rd;       // where the path ended: a point, or the direction it left along
#endif
    while (__ballot(live) != 0ull) {
        if (live) {
            closest_hit(r, a, stk, ro, rd, tg);
            live = false;
            fid = r.fid;
            if (fid < 0) {   // the path ends in a miss: the product and the distance stand
                nrm = v3(0.0f, 0.0f, 0.0f);
                mtl = -1;
#if TPT_AOV_PATH_POINTS
                end = rd;
#endif
            } else {
                float4 m0;
                Surf face;
                mtl = hit_prelude(a, r, nrm, m0, face);
                const float4 m1 = a.mtl[2 * mtl + 1];
                alb = alb * v3(m0.x, m0.y, m0.z);
                depth = depth + r.t;
#if TPT_AOV_PATH_POINTS
                end = ro + (r.t * rd);   // the advance below, whether or not the path goes on
#endif
                // new_direction's branch order (eta, then metallic); an emitter ends a path (:408-412)
                const bool mirror = !(m1.x > 0.0f) && m1.y > 0.0f && !(m0.w > 0.0f);
                if (mirror && k < p.max_bounces) {
                    ro = ro + (r.t * rd);   // k_trace's advance (:372)
                    rd = reflect_dir(rd, nrm);
                    tg = grazing(a.graze ? face : no_surface(), rd);
                    ++k;
                    live = true;
                }
            }
        }
    }
    // the statistics: one integer atomic each per wave over the spread counters
    const unsigned long long found = __ballot(k > 0);
    if (found) {   // (wave-uniform)
        int deep = k;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) deep = max(deep, __shfl_xor(deep, s, 64));
        if ((tid & 63) == 0) {
            atomicAdd(spread_slot(p.followed), (unsigned long long)__popcll(found));
            atomicMax(spread_slot(p.deepest), (unsigned long long)deep);
        }
    }
    if (!inside) return;
    const size_t off = (size_t)x + (size_t)y * (size_t)a.width;
    write_aov(o, off, alb, nrm, depth, fid, mtl);
    if (p.bounces) p.bounces[off] = k;
#if TPT_AOV_PATH_POINTS
    store3(points, off, end);
#endif
}
