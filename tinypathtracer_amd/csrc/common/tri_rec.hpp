// tri_rec.hpp -- the leaf triangle record (`tri`).
//
// Leaf slot j holds rayHitTriangle's operands (geometry_queries.h:65-86) for the
// triangle at sorted position j: v0, e1 = v1 - v0, e2 = v2 - v0 (pre-subtracted,
// the same rounding) and the face id, as three float4 at byte 48 j:
//   (v0.xyz, bits(fid)) (e1.xyz, 0) (e2.xyz, 0).
// (A packed 40-byte record was measured in round 5 -- C5 +0.3 %, C2 -0.6 %, C4
// within noise: the triangle bytes are not what C5 waits on -- and not kept.)
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace tpt {

constexpr int kTriFloats = 12;

// float4 units that hold n records
constexpr size_t tri_float4s(size_t n) { return (n * (size_t)kTriFloats + 3) / 4; }

// the record as rayHitTriangle's operands: q0 = (v0, bits(fid)), q1.xyz = e1, q2.xyz = e2
struct TriQ {
    float4 q0, q1, q2;
};

__device__ __forceinline__ TriQ tri_load(const float4* __restrict__ tri, int pos) {
    const float4* t = tri + 3 * (size_t)pos;
    return TriQ{t[0], t[1], t[2]};
}

__device__ __forceinline__ void tri_store(float4* tri, int pos, float v0x, float v0y, float v0z, int fid, float e1x,
                                          float e1y, float e1z, float e2x, float e2y, float e2z) {
    float4* t = tri + 3 * (size_t)pos;
    t[0] = make_float4(v0x, v0y, v0z, __int_as_float(fid));
    t[1] = make_float4(e1x, e1y, e1z, 0.0f);
    t[2] = make_float4(e2x, e2y, e2z, 0.0f);
}

}  // namespace tpt
