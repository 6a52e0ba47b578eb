// temporal_kernel.hpp -- k_temporal, one template for the eight temporal kernels.  post.hip includes
// it inside namespace tpt, behind the shared steps it calls.  The pack Ex is what a variant takes on
// top of TemporalArgs: nothing (tpt_temporal), MotionArgs (tpt_temporal_motion), TemporalPathArgs
// (tpt_temporal_path) or DeformArgs (tpt_temporal_deform), and behind any of these ClipArgs
// (tpt_history_set_clip).
#pragma once

// One lane per pixel, one launch per frame.  The lane reads its pixel of the caller's
// planes (3-float planes directly: a pack step would write and read them once more),
// gathers four taps of the previous state (three 16-B loads each, all issued before
// the first is used) and writes its pixel of the new state.  TILES = false: a wave is a 64-pixel row segment (block (64, 4)),
// so its own-pixel accesses are 1 KiB contiguous per float4 plane and its taps, which
// neighbouring lanes reproject to neighbouring addresses, nearly so; TILES = true:
// 16x16 tiles, each wave an 8x8 sub-tile as k_aov.  No LDS, no floating-point atomics.
//
// MOTION (MotionArgs mo; DESIGN.md section 5 "Moving objects"): a hit pixel
// also reads its face id, the face's object id and the object's record (MotionArgs), moves
// its world position by the object's D into the previous frame's world and turns its normal
// by G before the rules are applied.  Lanes of a wave mostly share an object, so the record's
// six 16-B loads are a broadcast from L2.  An object that did not move (kMotionIdentity) skips
// both products under its flag instead of multiplying by the unit matrix: 1 x + 0 y + 0 z + 0
// turns -0 into +0 and an infinite coordinate into NaN, while the skipped path leaves X and n
// as they are for every input, so that case is plain k_temporal's bit for bit.
//
// PATH (TemporalPathArgs pa; DESIGN.md section 5 "Temporal accumulation through
// mirrors"): the guides are the mirror-path ones, so X = ro + z rd is the virtual image of the
// path's terminal point.  The lane also reads its bounce count k (4 B) and, where k > 0, where
// its path ended (12 B).  A tap must hold the same k (the free fourth word of plane 2), and for
// k > 0 a terminal point (plane 3) within point_tol pixel footprints of the lane's own.  The
// plane-3 gathers are issued with the others, behind a wave-level ballot of k > 0: a wave
// without a mirror pixel moves plain k_temporal's bytes and the 4-byte k.  With k = 0 everywhere
// every added test passes and the arithmetic is plain k_temporal's: the same bits.
//
// DEFORM (DeformArgs de; DESIGN.md section 5 "Deforming meshes"): a hit pixel
// reads its face id, the face's three vertex indices and, per corner, the world position and
// normal as the scene holds them now and as the history's snapshot held them at the previous call:
// 3 + 36 words, the 36 issued together once the indices are there and ahead of their use, as the
// taps' loads are.  Neighbouring lanes share faces, so most of it is a broadcast from L2.  A
// triangle whose 18 words are bit-equal to the snapshot's takes plain k_temporal's path untouched (the
// test-and-skip that kMotionIdentity is for MOTION: with nothing deformed, the same
// bits).  Otherwise the pixel-centre ray's barycentrics on the current triangle (rayHitTriangle's
// arithmetic, geometry_queries.h:65-86, without its range tests) are applied to the snapshot's
// corners: X' is where that point of that triangle was, ne the normal it had.
//
// CLIP (ClipArgs cl, last in the pack; DESIGN.md section 5 "History clipping"): each of the four
// again, with one more argument.  The lane reads its pixel of k_clip_box's two planes with its first loads and,
// where it is reprojected, clamps the gathered history colour to the box before the blend; a
// history that the clamp moved is capped at clip_history frames and its luminance moments are
// shifted to the clamped colour's luminance at their variance.

struct NoArgs {};   // what a variant does not take: every use of it is inside a discarded `if constexpr`
template <class T, class... Ex>
constexpr bool has_v = (std::is_same_v<T, Ex> || ...);
template <class T>
constexpr bool temporal_kind_v = has_v<T, MotionArgs, TemporalPathArgs, DeformArgs>;
// the packs there are: (), (kind), (ClipArgs), (kind, ClipArgs)
template <class... Ex>
constexpr bool temporal_pack_v = sizeof...(Ex) == 0;
template <class E>
constexpr bool temporal_pack_v<E> = temporal_kind_v<E> || std::is_same_v<E, ClipArgs>;
template <class E>
constexpr bool temporal_pack_v<E, ClipArgs> = temporal_kind_v<E>;
static_assert(temporal_pack_v<> && temporal_pack_v<ClipArgs> && temporal_pack_v<DeformArgs, ClipArgs> &&
              !temporal_pack_v<ClipArgs, DeformArgs> && !temporal_pack_v<MotionArgs, TemporalPathArgs> &&
              !temporal_pack_v<ClipArgs, ClipArgs> && !temporal_pack_v<TemporalArgs>, "temporal_pack_v");

// The argument of type T, or NoArgs where the pack has none.
template <class T>
__device__ __forceinline__ NoArgs pick() {
    return NoArgs{};
}
template <class T, class E, class... Ex>
__device__ __forceinline__ decltype(auto) pick(const E& e, const Ex&... ex) {
    if constexpr (std::is_same_v<T, E>) return (e);
    else return pick<T>(ex...);
}

template <bool TILES, class... Ex>
__global__ __launch_bounds__(256) void k_temporal(TemporalArgs a, Ex... ex) {
    static_assert(temporal_pack_v<Ex...>, "at most one of MotionArgs, TemporalPathArgs, DeformArgs, then at most one ClipArgs");
    constexpr bool MOTION = has_v<MotionArgs, Ex...>, PATH = has_v<TemporalPathArgs, Ex...>,
                   DEFORM = has_v<DeformArgs, Ex...>, CLIP = has_v<ClipArgs, Ex...>;
    const auto& mo = pick<MotionArgs>(ex...);
    const auto& pa = pick<TemporalPathArgs>(ex...);
    const auto& de = pick<DeformArgs>(ex...);
    const auto& cl = pick<ClipArgs>(ex...);
    // face, n_faces and motion_out, which MotionArgs and DeformArgs both hold
    const auto& fm = pick<std::conditional_t<DEFORM, DeformArgs, MotionArgs>>(ex...);
    int x, y, tid;
    if (TILES) {
        tid = (int)threadIdx.x;
        const int2 xy = tile_wave_xy(tid);
        x = xy.x;
        y = xy.y;
    } else {
        tid = (int)threadIdx.y * 64 + (int)threadIdx.x;
        x = (int)blockIdx.x * 64 + (int)threadIdx.x;
        y = (int)blockIdx.y * 4 + (int)threadIdx.y;
    }
    bool reproj = false, clipped = false;
    if (x < a.width && y < a.height) {
        const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
        // what the reprojection needs first, so that the taps' loads start early
        const float z = a.depth[p];
        const int m = a.material[p];
        // (blo, bhi, kb and face, which only some variants read, get their one value in the variant's
        // block, kb ahead of pe: a neutral value first, or kb's load behind pe, and the path, deform
        // and clip kernels' instructions are no longer what they were, tools/kernel_diff.py)
        float4 blo, bhi;
        if constexpr (CLIP) {                              // the box: own-pixel loads, in flight with the first
            blo = cl.lo[p];
            bhi = cl.hi[p];
        }
        int kb;
        if constexpr (PATH) kb = pa.bounces[p];
        V3 pe = v3(0.0f, 0.0f, 0.0f);                      // where the path ended (k > 0 only)
        if constexpr (PATH) {
            if (kb > 0) pe = v3(pa.points[3 * p], pa.points[3 * p + 1], pa.points[3 * p + 2]);
        }
        int face;
        if constexpr (MOTION || DEFORM) face = fm.face[p];
        float mvx = 0.0f, mvy = 0.0f;                      // where the pixel came from, minus where it is
        const V3 n = v3(a.normal[3 * p], a.normal[3 * p + 1], a.normal[3 * p + 2]);
        const V3 in = v3(a.radiance_in[3 * p], a.radiance_in[3 * p + 1], a.radiance_in[3 * p + 2]);
        V3 alb = v3(1.0f, 1.0f, 1.0f);
        if (a.demodulate) alb = v3(a.albedo[3 * p], a.albedo[3 * p + 1], a.albedo[3 * p + 2]);
        const bool hit = m >= 0;
        float4 hc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // history: colour, N
        float hm1 = 0.0f, hm2 = 0.0f;
        if (a.has_prev) {
            V3 ro, rd;   // the pixel-centre ray of the current camera: k_aov's
            centre_ray(a, x, y, ro, rd);
            // a hit reprojects its world position, a miss its direction (a point at infinity)
            V3 X = hit ? ro + (z * rd) : rd;
            V3 ne = n;                                     // the normal as the previous frame held it
            bool tracked = true;
            if constexpr (DEFORM) {
                if (hit) {
                    // (the face id is compared before it indexes anything)
                    tracked = de.snap_valid != 0 && (unsigned)face < (unsigned)fm.n_faces;
                    if (tracked) {
                        const uint32_t* ix = de.indices + 3 * (size_t)face;
                        const size_t i0 = 3 * (size_t)ix[0], i1 = 3 * (size_t)ix[1], i2 = 3 * (size_t)ix[2];
                        // all 36 words before the first is used: one round trip, not twelve
                        float cv[9], pv[9], pn[9], cn[9];
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            cv[k] = de.wverts[i0 + k];
                            cv[3 + k] = de.wverts[i1 + k];
                            cv[6 + k] = de.wverts[i2 + k];
                            pv[k] = de.prev_wverts[i0 + k];
                            pv[3 + k] = de.prev_wverts[i1 + k];
                            pv[6 + k] = de.prev_wverts[i2 + k];
                            pn[k] = de.prev_wnorms[i0 + k];
                            pn[3 + k] = de.prev_wnorms[i1 + k];
                            pn[6 + k] = de.prev_wnorms[i2 + k];
                            cn[k] = de.wnorms[i0 + k];
                            cn[3 + k] = de.wnorms[i1 + k];
                            cn[6 + k] = de.wnorms[i2 + k];
                        }
                        int differ = 0;
#pragma unroll
                        for (int k = 0; k < 9; ++k)
                            differ |= (__float_as_int(cv[k]) ^ __float_as_int(pv[k])) | (__float_as_int(cn[k]) ^ __float_as_int(pn[k]));
                        if (differ != 0) {
                            const V3 v0 = v3(cv[0], cv[1], cv[2]);
                            const V3 e1 = v3(cv[3], cv[4], cv[5]) - v0, e2 = v3(cv[6], cv[7], cv[8]) - v0;
                            const V3 tv = ro - v0;
                            const V3 pp = cross(rd, e2);
                            const V3 qq = cross(tv, e1);
                            const float denom = dot(pp, e1);
                            const float id = 1.0f / denom;
                            const float u = dot(pp, tv) * id;
                            const float v = dot(qq, rd) * id;
                            const float w = 1.0f - u - v;
                            X = ((w * v3(pv[0], pv[1], pv[2])) + (u * v3(pv[3], pv[4], pv[5]))) + (v * v3(pv[6], pv[7], pv[8]));
                            const V3 gn = ((w * v3(pn[0], pn[1], pn[2])) + (u * v3(pn[3], pn[4], pn[5]))) + (v * v3(pn[6], pn[7], pn[8]));
                            // a square root and divisions, not frsqrt: its 2e-3 would decide the normal rule
                            const float len = fsqrt(norm2(gn));
                            ne = v3(gn.x / len, gn.y / len, gn.z / len);
                            // a flat triangle (the determinant the triangle test rejects) and whatever is
                            // not finite: u and v in X' make it non-finite when they are
                            tracked = denom != 0.0f && __builtin_isfinite(u) && __builtin_isfinite(v) &&
                                      __builtin_isfinite(X.x) && __builtin_isfinite(X.y) && __builtin_isfinite(X.z);
                        }
                    }
                }
            } else if constexpr (MOTION) {
                if (hit) {
                    tracked = (unsigned)face < (unsigned)fm.n_faces;   // compared before it indexes anything
                    if (tracked) {
                        const float4* rec = mo.records + 6 * (size_t)mo.face_object[face];
                        const float4 d0 = rec[0], d1 = rec[1], d2 = rec[2], g0 = rec[3], g1 = rec[4], g2 = rec[5];
                        const int flag = __float_as_int(g2.y);
                        tracked = flag != kMotionUntracked;
                        if (flag == kMotionTracked) {
                            X = v3(((d0.x * X.x + d0.y * X.y) + d0.z * X.z) + d0.w,
                                   ((d1.x * X.x + d1.y * X.y) + d1.z * X.z) + d1.w,
                                   ((d2.x * X.x + d2.y * X.y) + d2.z * X.z) + d2.w);
                            const V3 gn = v3((g0.x * n.x + g0.y * n.y) + g0.z * n.z, (g0.w * n.x + g1.x * n.y) + g1.y * n.z,
                                             (g1.z * n.x + g1.w * n.y) + g2.x * n.z);
                            // a square root and divisions, not frsqrt: its 2e-3 would decide the normal rule
                            const float len = fsqrt(norm2(gn));
                            ne = v3(gn.x / len, gn.y / len, gn.z / len);
                        }
                    }
                }
            }
            float loc[4];
            mat4_vec4(a.prev_inv, X.x, X.y, X.z, hit ? 1.0f : 0.0f, loc);
            float dist = 0.0f;
            if (hit) dist = fsqrt(norm2(X - v3(a.prev_origin[0], a.prev_origin[1], a.prev_origin[2])));
            if (loc[2] < 0.0f && tracked) {
                const float s = -1.0f / loc[2];
                float fx = (loc[0] * s + a.prev_half_sw) / a.prev_sensor_w * (float)a.width - 0.5f;
                float fy = (loc[1] * s + a.prev_half_sh) / a.prev_sensor_h * (float)a.height - 0.5f;
                const float rx = rintf(fx), ry = rintf(fy);
                if (fabsf(fx - rx) < kSnap) fx = rx;
                if (fabsf(fy - ry) < kSnap) fy = ry;
                if constexpr (MOTION || DEFORM) {
                    if (__builtin_isfinite(fx) && __builtin_isfinite(fy)) {
                        mvx = fx - (float)x;
                        mvy = fy - (float)y;
                    }
                }
                // some tap of positive weight inside the frame (false for NaN and out-of-range values too)
                if (fx > -1.0f && fx < (float)a.width && fy > -1.0f && fy < (float)a.height) {
                    const float x0f = floorf(fx), y0f = floorf(fy);
                    const float tx = fx - x0f, ty = fy - y0f;
                    const int x0 = (int)x0f, y0 = (int)y0f;
                    // The four taps' weights and addresses first, then all twelve loads, then the
                    // tests: the loads are in flight together (a chain of dependent, conditional
                    // loads measured 0.40 ms at 1080p, latency-bound).  A tap of weight 0 or outside
                    // the frame is never read: its loads go to the lane's own pixel instead.
                    float w[4];
                    size_t q[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int qx = x0 + (t & 1), qy = y0 + (t >> 1);
                        w[t] = ((t & 1) ? tx : 1.0f - tx) * ((t >> 1) ? ty : 1.0f - ty);
                        if (!(w[t] > 0.0f) || qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) w[t] = 0.0f;
                        q[t] = w[t] > 0.0f ? (size_t)qy * (size_t)a.width + (size_t)qx : p;
                    }
                    float4 s0[4], s1[4], s2[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        s2[t] = a.prev[2][q[t]];
                        s1[t] = a.prev[1][q[t]];
                        s0[t] = a.prev[0][q[t]];
                    }
                    float4 s3[4];
                    float ptol = 0.0f;
                    if constexpr (PATH) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) s3[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if (__ballot(kb > 0) != 0ull) {        // (wave-level: no mirror pixel, no plane-3 traffic)
                            if (kb > 0) {
#pragma unroll
                                for (int t = 0; t < 4; ++t) s3[t] = pa.prev_points[q[t]];
                            }
                        }
                        // the point rule's radius: point_tol footprints at the path's length; a direction's at 1
                        ptol = (pa.point_tol * (hit ? z : 1.0f)) * a.sensor_h * a.inv_h;
                    }
                    float wsum = 0.0f;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        bool ok = w[t] > 0.0f && __float_as_int(s2[t].z) == m;
                        if constexpr (PATH) {
                            ok = ok && __float_as_int(s2[t].w) == kb;
                            if (kb > 0) ok = ok && fsqrt(norm2(v3(s3[t].x, s3[t].y, s3[t].z) - pe)) <= ptol;
                        }
                        if (hit) {
                            const float4 g = s1[t];
                            ok = ok && fabsf(g.w - dist) <= a.depth_tol * dist &&
                                 (g.x * ne.x + g.y * ne.y) + g.z * ne.z >= a.normal_min;
                        }
                        if (!ok) continue;
                        wsum += w[t];
                        hc.x += w[t] * s0[t].x;
                        hc.y += w[t] * s0[t].y;
                        hc.z += w[t] * s0[t].z;
                        hc.w += w[t] * s0[t].w;
                        hm1 += w[t] * s2[t].x;
                        hm2 += w[t] * s2[t].y;
                    }
                    if (wsum >= kMinWsum) {
                        reproj = true;
                        // divisions, not a reciprocal: taps of one history length N' give N' exactly
                        hc = make_float4(hc.x / wsum, hc.y / wsum, hc.z / wsum, hc.w / wsum);
                        hm1 = hm1 / wsum;
                        hm2 = hm2 / wsum;
                    }
                }
            }
        }
        V3 c = in;
        if (a.demodulate) {
            alb = v3(albedo_floor(alb.x), albedo_floor(alb.y), albedo_floor(alb.z));
            c = v3(in.x / alb.x, in.y / alb.y, in.z / alb.z);
        }
        const float L = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
        // disoccluded: selected, not blended -- the colour and the output are the input bit for bit
        float N = 1.0f, m1 = L, m2 = L * L;
        V3 C = c, out = in;
        if (reproj) {
            if constexpr (CLIP) {
                // (fmaxf / fminf return the other operand for a NaN one: a NaN edge leaves the value as it is)
                const V3 hcl = v3(fminf(fmaxf(hc.x, blo.x), bhi.x), fminf(fmaxf(hc.y, blo.y), bhi.y),
                                  fminf(fmaxf(hc.z, blo.z), bhi.z));
                clipped = hcl.x != hc.x || hcl.y != hc.y || hcl.z != hc.z;
                if (clipped) {
                    hc = make_float4(hcl.x, hcl.y, hcl.z, fminf(hc.w, cl.clip_history));
                    // the accumulated variance moves with the mean
                    const float v = fmaxf(hm2 - hm1 * hm1, 0.0f);
                    hm1 = (0.2126f * hcl.x + 0.7152f * hcl.y) + 0.0722f * hcl.z;
                    hm2 = v + hm1 * hm1;
                }
            }
            N = fminf(hc.w + 1.0f, a.max_history);
            const float k = fmaxf(a.alpha, 1.0f / N);
            C = v3(hc.x + k * (c.x - hc.x), hc.y + k * (c.y - hc.y), hc.z + k * (c.z - hc.z));
            m1 = hm1 + k * (m1 - hm1);
            m2 = hm2 + k * (m2 - hm2);
            out = a.demodulate ? C * alb : C;
        }
        a.next[0][p] = make_float4(C.x, C.y, C.z, N);
        a.next[1][p] = make_float4(n.x, n.y, n.z, z);
        if constexpr (PATH) {
            a.next[2][p] = make_float4(m1, m2, __int_as_float(m), __int_as_float(kb));
            if (kb > 0) pa.next_points[p] = make_float4(pe.x, pe.y, pe.z, 0.0f);
        } else {
            a.next[2][p] = make_float4(m1, m2, __int_as_float(m), 0.0f);
        }
        if (a.radiance_out) {
            a.radiance_out[3 * p] = out.x;
            a.radiance_out[3 * p + 1] = out.y;
            a.radiance_out[3 * p + 2] = out.z;
        }
        if (a.variance_out) a.variance_out[p] = fmaxf(m2 - m1 * m1, 0.0f);
        if (a.history_out) a.history_out[p] = N;
        if constexpr (MOTION || DEFORM) {
            if (fm.motion_out) {
                fm.motion_out[2 * p] = mvx;
                fm.motion_out[2 * p + 1] = mvy;
            }
        }
        if (a.bgra) write_bgr(a.bgra, a.width, a.height, (size_t)x, (size_t)y, out);
    }
    spread_count(a.reprojected, tid, reproj);   // the statistic
    if constexpr (CLIP) spread_count(cl.clipped, tid, clipped);
}
