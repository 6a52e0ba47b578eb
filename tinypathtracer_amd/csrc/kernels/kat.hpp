// kat.hpp -- launcher of the env / sampler known-answer kernel (kat.hip,
// tpt_debug_env_kat).  A header of its own: the trace kernels do not see it.
#pragma once

#include "../common/device_api.hpp"

namespace tpt {

constexpr int kEnvKatOps = 6;
// floats per case read from `in` and written to `out`, by op (layouts: tpt.h)
constexpr int kEnvKatIn[kEnvKatOps] = {1, 2, 1, 3, 5, 8};
constexpr int kEnvKatOut[kEnvKatOps] = {2, 1, 1, 10, 7, 5};

// a: only the env fields are read (ops 3 and 4).  state: 6 words per case, op 5 only.
hipError_t launch_env_kat(const TraceArgs& a, int op, uint32_t n, const float* in, uint32_t* state, float* out,
                          hipStream_t s);

}  // namespace tpt
