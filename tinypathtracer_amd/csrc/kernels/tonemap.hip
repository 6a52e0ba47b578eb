// tonemap.hip -- the display stage behind the post-pass (tpt_tonemap; DESIGN.md section 5 "Tone
// mapping"): exposure, tone curve, transfer function and rounding to bytes.  Built with post.hip's
// flags: no FMA contraction, so the luminance and the bins are numpy float32's bit for bit.
//
//  * k_tm_hist: the luminance histogram of a frame, 256 bins of 1/8 octave read from the float's
//    own bits.  A capped grid-stride grid (kHistMaxBlocks workgroups of 256 lanes); a workgroup
//    counts in LDS and writes its 256 counts to its own row of the partials: no global atomic,
//    no floating-point atomic.  Lanes of a wave that hold the same bin add once (hist_add).
//  * k_tm_measure: one workgroup.  Column sums of the partials, the integer prefix sum in LDS,
//    the trimmed log-average in double, the exposure's update.  It leaves the scale in device
//    memory, where the map kernel reads it: the value never visits the host in between.
//  * k_tonemap: one lane per pixel, a wave a 64-pixel row segment (block (64, 4)) as k_temporal's
//    row layout.  Reads 12 B, writes 12 B of floats, 3 bytes, or both.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "device_api.hpp"

namespace tpt {

// k_temporal's and the variance-guided filter's L (post.hip svgf_lum), the same arithmetic.
__device__ __forceinline__ float tm_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// ---- the histogram ----

constexpr int kBinNone = -1;             // no pixel, or a dark one (L < 2^-16: counted by subtraction)
constexpr int kBinNan = 256;             // the LDS counter behind the 256 bins
constexpr int kHistPeel = 4;             // rounds of hist_add's aggregation
constexpr int kHistUnroll = 4;           // pixels a lane loads before it counts the first

// bin = clamp(8 (e + 16) + m3, 0, 255) of L >= 2^-16, e the unbiased exponent, m3 the top three
// mantissa bits; +inf and L >= 2^16 go to bin 255.
__device__ __forceinline__ int lum_bin(float L) {
    if (L != L) return kBinNan;
    if (!(L >= 0x1p-16f)) return kBinNone;
    if (L >= 0x1p16f) return 255;
    const uint32_t u = __float_as_uint(L);
    return 8 * ((int)(u >> 23) - 127 + 16) + (int)((u >> 20) & 7u);
}

// One count per lane into the workgroup's LDS histogram.  A constant frame would send all 64
// lanes of a wave to one LDS counter, which the LDS serialises: up to kHistPeel times the wave
// takes the bin of its first remaining lane and adds the number of lanes that hold it in one
// add; what is left after that (a noisy wave) adds lane by lane.  Called by whole waves.
__device__ __forceinline__ void hist_add(uint32_t* h, int bin, int lane) {
#pragma unroll
    for (int r = 0; r < kHistPeel; ++r) {
        const unsigned long long live = __ballot(bin >= 0);
        if (!live) return;
        const int leader = __ffsll(live) - 1;
        const int b0 = __builtin_amdgcn_readlane(bin, leader);
        const unsigned long long same = __ballot(bin == b0);
        if (lane == leader) atomicAdd(&h[b0], (uint32_t)__popcll(same));
        if (bin == b0) bin = kBinNone;
    }
    if (bin >= 0) atomicAdd(&h[bin], 1u);
}

__global__ __launch_bounds__(256) void k_tm_hist(HistArgs a) {
    __shared__ uint32_t h[kBinNan + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    for (int i = tid; i <= kBinNan; i += 256) h[i] = 0u;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * 256;
    // the bound is the workgroup's, so that whole waves reach hist_add
    for (size_t base = (size_t)blockIdx.x * 256; base < a.npix; base += (size_t)kHistUnroll * stride) {
        int bin[kHistUnroll];
#pragma unroll
        for (int u = 0; u < kHistUnroll; ++u) {
            const size_t p = base + (size_t)u * stride + (size_t)tid;
            bin[u] = kBinNone;
            if (p < a.npix) bin[u] = lum_bin(tm_lum(a.radiance[3 * p], a.radiance[3 * p + 1], a.radiance[3 * p + 2]));
        }
#pragma unroll
        for (int u = 0; u < kHistUnroll; ++u) hist_add(h, bin[u], lane);
    }
    __syncthreads();
    a.partials[(size_t)blockIdx.x * kHistRowWords + (size_t)tid] = h[tid];
    if (tid == 0) a.partials[(size_t)kHistMaxBlocks * kHistRowWords + blockIdx.x] = h[kBinNan];
}

// ---- the measurement ----

// The partials were written by every XCD, so one workgroup reads them at the latency of the
// fabric: 16 waves read them, wave w the rows w, w + 16, ... as one 16-B load per lane (a row is
// 1 KiB: one load of a wave) with eight in flight (measured at 1920x1080, 512 rows: 0.118 ms with
// one lane per column, 0.039 ms with four, eight 4-B loads in flight each).  The first 256 lanes
// (`lead`) do the rest, and every lane passes every barrier.
constexpr int kMeasureWaves = 16;
static_assert(kHistRowWords == 4 * 64, "a wave reads a row as 64 uint4");

__global__ __launch_bounds__(64 * kMeasureWaves) void k_tm_measure(MeasureArgs a) {
    __shared__ unsigned long long c[256];    // the inclusive prefix sums of the bins
    __shared__ unsigned long long nf[256];   // the NaN counts
    __shared__ double t[256];                // overlap_k rep_k
    __shared__ unsigned long long part[kMeasureWaves][256];
    const int k = (int)threadIdx.x & 255, wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const bool lead = threadIdx.x < 256;
    {
        const uint4* rows = reinterpret_cast<const uint4*>(a.partials);
        unsigned long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll 8
        for (int b = wave; b < a.blocks; b += kMeasureWaves) {
            const uint4 v = rows[(size_t)b * (kHistRowWords / 4) + (size_t)lane];
            s0 += v.x;
            s1 += v.y;
            s2 += v.z;
            s3 += v.w;
        }
        part[wave][4 * lane] = s0;
        part[wave][4 * lane + 1] = s1;
        part[wave][4 * lane + 2] = s2;
        part[wave][4 * lane + 3] = s3;
    }
    __syncthreads();
    unsigned long long hk = 0, n = 0;
#pragma unroll
    for (int w = 0; w < kMeasureWaves; ++w) hk += part[w][k];
    if (lead) {
        for (int b = k; b < a.blocks; b += 256) n += a.partials[(size_t)kHistMaxBlocks * kHistRowWords + (size_t)b];
        c[k] = hk;
        nf[k] = n;
    }
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        unsigned long long v = c[k];
        if (k >= d) v += c[k - d];
        __syncthreads();
        if (lead) c[k] = v;
        __syncthreads();
    }
    const unsigned long long N = c[255], Ck = c[k] - hk;
    // the pixels between the shares p_low and p_high of the counted ones, and this bin's part of them
    const double lo = floor(a.p_low * (double)N), hi = fmax(ceil(a.p_high * (double)N), lo + 1.0);
    const double overlap = fmax(0.0, fmin((double)(Ck + hk), hi) - fmax((double)Ck, lo));
    const double rep = (double)(k / 8 - 16) + log2(1.0 + ((double)(k % 8) + 0.5) / 8.0);
    if (lead) t[k] = overlap * rep;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {   // a fixed order: the same bits every call
        if (lead && k < d) {
            t[k] += t[k + d];
            nf[k] += nf[k + d];
        }
        __syncthreads();
    }
    if (lead) a.block->hist[k] = hk;
    if (threadIdx.x == 0) {
        double s = a.has_state ? a.block->s : 0.0, log2_avg = 0.0;
        if (N > 0) {
            log2_avg = t[0] / (hi - lo);
            const double target = fmin(fmax(log2(a.key) - log2_avg, a.min_ev), a.max_ev);
            s = a.has_state ? s + a.rate * (target - s) : target;
            a.block->s = s;
        }
        const float log2_scale = (float)(s + a.ev);
        a.block->log2_scale = log2_scale;
        a.block->scale = exp2f(log2_scale);
        a.block->log2_avg = (float)log2_avg;
        a.block->counted = N;
        a.block->nonfinite = nf[0];
        a.block->dark = (unsigned long long)a.npix - N - nf[0];
    }
}

// ---- the map ----

// The 4x4 Bayer matrix, row-major in nibbles from the lowest:
//    0  8  2 10 / 12  4 14  6 /  3 11  1  9 / 15  7 13  5
constexpr unsigned long long kBayer4 = 0x5D7F91B36E4CA280ull;

// y^e of y in [0, 1], e > 0, by the hardware's log2 and exp2 (one ulp each).  With u = e |log2 y|
// the result is 2^-u, and an ulp of log2 y moves it by 2^-u u 2^-23 ln 2 <= 5e-8 (u 2^-u <= 0.54);
// the product's and exp2's own ulps add about 1.2e-7 of the result.  powf's extra instructions per
// channel made the kernel compute-bound (0.028 ms against 0.025 ms for k_upsample).  y = 0 gives 0.
__device__ __forceinline__ float tm_pow(float y, float e) { return __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(y) * e); }

__device__ __forceinline__ float tm_transfer(float y, int transfer, float inv_gamma) {
    if (transfer == 1) y = y <= 0.0031308f ? 12.92f * y : 1.055f * tm_pow(y, 1.0f / 2.4f) - 0.055f;
    else if (transfer == 2) y = tm_pow(y, inv_gamma);
    return fminf(fmaxf(y, 0.0f), 1.0f);
}

__device__ __forceinline__ uint8_t tm_byte(float y, float d) {   // floor(clamp(255 y + 0.5 + d, 0, 255))
    return (uint8_t)fminf(fmaxf(255.0f * y + (0.5f + d), 0.0f), 255.0f);
}

__global__ __launch_bounds__(256) void k_tonemap(TonemapArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (x >= a.width) return;
    const float scale = a.block ? a.block->scale : a.scale;
    for (int y = (int)blockIdx.y * 4 + (int)threadIdx.y; y < a.height; y += (int)gridDim.y * 4) {
        const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
        // x = min(max(c scale, 0), 65504): fmaxf gives 0 for a NaN
        const float r = fminf(fmaxf(a.radiance_in[3 * p] * scale, 0.0f), 65504.0f);
        const float g = fminf(fmaxf(a.radiance_in[3 * p + 1] * scale, 0.0f), 65504.0f);
        const float b = fminf(fmaxf(a.radiance_in[3 * p + 2] * scale, 0.0f), 65504.0f);
        float yr, yg, yb;
        if (a.op == 1) {   // extended Reinhard on luminance: x Ly / Lx, Ly = Lx (1 + Lx / white^2) / (1 + Lx)
            const float Lx = tm_lum(r, g, b);
            const float k = Lx > 0.0f ? (1.0f + Lx / a.white2) / (1.0f + Lx) : 0.0f;
            yr = fminf(fmaxf(r * k, 0.0f), 1.0f);
            yg = fminf(fmaxf(g * k, 0.0f), 1.0f);
            yb = fminf(fmaxf(b * k, 0.0f), 1.0f);
        } else if (a.op == 2) {   // Narkowicz 2015
            yr = fminf(fmaxf(r * (2.51f * r + 0.03f) / (r * (2.43f * r + 0.59f) + 0.14f), 0.0f), 1.0f);
            yg = fminf(fmaxf(g * (2.51f * g + 0.03f) / (g * (2.43f * g + 0.59f) + 0.14f), 0.0f), 1.0f);
            yb = fminf(fmaxf(b * (2.51f * b + 0.03f) / (b * (2.43f * b + 0.59f) + 0.14f), 0.0f), 1.0f);
        } else {
            yr = fminf(r, 1.0f);
            yg = fminf(g, 1.0f);
            yb = fminf(b, 1.0f);
        }
        yr = tm_transfer(yr, a.transfer, a.inv_gamma);
        yg = tm_transfer(yg, a.transfer, a.inv_gamma);
        yb = tm_transfer(yb, a.transfer, a.inv_gamma);
        if (a.radiance_out) {
            a.radiance_out[3 * p] = yr;
            a.radiance_out[3 * p + 1] = yg;
            a.radiance_out[3 * p + 2] = yb;
        }
        if (a.bgra) {   // tpt_denoise's layout: row 0 = top, B, G, R written, alpha untouched
            float d = 0.0f;
            if (a.dither) d = ((float)((kBayer4 >> (4 * ((y & 3) * 4 + (x & 3)))) & 15ull) + 0.5f) / 16.0f - 0.5f;
            uint8_t* px = a.bgra + 4 * (((size_t)a.height - (size_t)y - 1) * (size_t)a.width + (size_t)x);
            px[0] = tm_byte(yb, d);
            px[1] = tm_byte(yg, d);
            px[2] = tm_byte(yr, d);
        }
    }
}

int hist_blocks(size_t npix) { return (int)std::min<size_t>((size_t)kHistMaxBlocks, (npix + 255) / 256); }

hipError_t launch_histogram(const HistArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_tm_hist, dim3((unsigned)a.blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_measure(const MeasureArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_tm_measure, dim3(1), dim3(64 * kMeasureWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tonemap(const TonemapArgs& a, hipStream_t s) {
    const unsigned rows = (unsigned)((a.height + 3) / 4);
    hipLaunchKernelGGL(k_tonemap, dim3((unsigned)((a.width + 63) / 64), std::min(rows, 65535u)), dim3(64, 4), 0, s, a);
    return hipGetLastError();
}

}  // namespace tpt
