// kat.hip -- known-answer kernel over the device functions of trace_dev.hpp that
// the hot-path KATs of trace.hip (k_hot_kat) do not reach: the parity trig as the
// device compiles it, the env lookup's texel indices (fast and exact), env
// importance sampling against an env's real device tables, and getNewDirection.
// Tests only (tpt_debug_env_kat; tests/test_gpu_env_maps.py compares every output
// bit for bit with the oracle's hooks).  One case per lane; layouts: tpt.h.
#include "kat.hpp"
#include "trace_dev.hpp"

namespace tpt {

__global__ __launch_bounds__(256) void k_env_kat(TraceArgs a, int op, uint32_t n, const float* __restrict__ in,
                                                 uint32_t* __restrict__ state, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (op == 0) {
        float s, c;
        fsincos_2pi(in[i], s, c);
        out[2 * (size_t)i] = s;
        out[2 * (size_t)i + 1] = c;
    } else if (op == 1) {
        out[i] = patan2_fast(in[2 * (size_t)i], in[2 * (size_t)i + 1]);
    } else if (op == 2) {
        out[i] = pacos_fast(in[i]);
    } else if (op == 3) {
        const float* c = in + 3 * (size_t)i;
        const V3 d = v3(c[0], c[1], c[2]);
        float* q = out + 10 * (size_t)i;
        q[0] = (float)env_col_fast(d.z, d.x, a.env_w);
        q[1] = (float)env_row_fast(d.y, a.env_h);
        q[2] = (float)env_col_exact(d.z, d.x, a.env_w);
        q[3] = (float)env_row_exact(d.y, a.env_h);
        const V3 le = env_lookup<false>(a.env, a.env_w, a.env_h, d);   // the variants without env IS
        q[4] = le.x;
        q[5] = le.y;
        q[6] = le.z;
        const V3 li = env_lookup<true>(a.env, a.env_w, a.env_h, d);    // the env-IS variants' inlined form
        q[7] = li.x;
        q[8] = li.y;
        q[9] = li.z;
    } else if (op == 4) {
        const float* c = in + 5 * (size_t)i;
        V3 dir = v3(0.0f, 0.0f, 0.0f), k_le = v3(0.0f, 0.0f, 0.0f);
        const bool ok = env_is_sample(a, v3(c[0], c[1], c[2]), c[3], c[4], dir, k_le);
        if (!ok) k_le = v3(0.0f, 0.0f, 0.0f);
        float* q = out + 7 * (size_t)i;
        q[0] = ok ? 1.0f : 0.0f;
        q[1] = dir.x;
        q[2] = dir.y;
        q[3] = dir.z;
        q[4] = k_le.x;
        q[5] = k_le.y;
        q[6] = k_le.z;
    } else if (op == 5) {
        const float* c = in + 8 * (size_t)i;
        uint32_t st[6];
        for (int k = 0; k < 6; ++k) st[k] = state[6 * (size_t)i + k];
        V3 next = v3(0.0f, 0.0f, 0.0f);
        float atten = 0.0f;
        const float pdf = new_direction(v3(c[0], c[1], c[2]), v3(c[3], c[4], c[5]), c[6], c[7], st, next, atten);
        for (int k = 0; k < 6; ++k) state[6 * (size_t)i + k] = st[k];
        float* q = out + 5 * (size_t)i;
        q[0] = next.x;
        q[1] = next.y;
        q[2] = next.z;
        q[3] = atten;
        q[4] = pdf;
    }
}

hipError_t launch_env_kat(const TraceArgs& a, int op, uint32_t n, const float* in, uint32_t* state, float* out,
                          hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_env_kat, dim3((n + 255) / 256), dim3(256), 0, s, a, op, n, in, state, out);
    return hipGetLastError();
}

}  // namespace tpt
