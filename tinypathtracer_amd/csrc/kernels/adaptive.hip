// adaptive.hip -- the kernels of tpt_render_adaptive beside k_trace's listed launches
// (DESIGN.md section 5 "Adaptive sampling"): the error estimate of a list of 16x16-pixel
// tiles and the resolve of a frame whose tiles hold different sample counts.
//
// The estimate is the criterion of Dammertz et al., "A Hierarchical Automatic Stopping
// Condition for Monte Carlo Global Illumination" (2010), with the first half of a pixel's
// samples as the half buffer: I = the n-spp radiance, A = the n/2-spp radiance,
//   e = (|I.r - A.r| + |I.g - A.g| + |I.b - A.b|) / sqrt(max(I.r + I.g + I.b, 1e-4)),
// and a tile's error is the mean of e over its in-frame pixels.
#include "trace_dev.hpp"

namespace tpt {

// One 256-lane workgroup per listed tile, lane (tid & 15, tid >> 4) on the tile's pixel.
// The sum runs in a fixed order -- within a wave by halving (lane i += lane i + 32, 16, ...,
// 1), then waves 0..3 in order through LDS -- without floating-point atomics, so the
// estimate is deterministic.  A non-finite pixel makes its tile's error NaN (inf - inf, or
// inf / sqrt(inf)); NaN is below no target, so the host runs such a tile to max_spp.
// Each lane reads its pixel's sums and snapshot before it overwrites the snapshot.
__global__ __launch_bounds__(256) void k_tile_error(TileErrorArgs a) {
    __shared__ float s_wave[4];
    const int tid = threadIdx.x;
    const uint32_t t = a.tile_list[blockIdx.x];
    const int tx = (int)(t & 0xffffu), ty = (int)(t >> 16);
    const int x = tx * 16 + (tid & 15), y = ty * 16 + (tid >> 4);
    const bool pixel = x < a.width && y < a.height;
    const size_t npix = (size_t)a.width * (size_t)a.height;
    const size_t off = pixel ? (size_t)x + (size_t)y * (size_t)a.width : 0;
    float e = 0.0f;
    if (pixel) {
        const float sr = a.accum[off], sg = a.accum[npix + off], sb = a.accum[2 * npix + off];
        if (!a.snapshot_only) {
            // k_resolve's arithmetic: I is the pixel's n-spp radiance to the bit
            const float inv = 1.0f / (float)a.n, inv_half = 1.0f / (float)(a.n / 2);
            const float ir = (0.0f + sr) * inv, ig = (0.0f + sg) * inv, ib = (0.0f + sb) * inv;
            const float ar = (0.0f + a.snapshot[off]) * inv_half, ag = (0.0f + a.snapshot[npix + off]) * inv_half,
                        ab = (0.0f + a.snapshot[2 * npix + off]) * inv_half;
            e = (fabsf(ir - ar) + fabsf(ig - ag) + fabsf(ib - ab)) / sqrtf(fmaxf(ir + ig + ib, 1e-4f));
        }
        a.snapshot[off] = sr;
        a.snapshot[npix + off] = sg;
        a.snapshot[2 * npix + off] = sb;
    }
    if (a.snapshot_only) return;   // (uniform)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) e += __shfl_down(e, d, 64);
    if ((tid & 63) == 0) s_wave[tid >> 6] = e;
    __syncthreads();
    if (tid == 0) {
        const int nx = min(16, a.width - tx * 16), ny = min(16, a.height - ty * 16);
        const float sum = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
        a.tile_error[(size_t)ty * (size_t)a.tiles_x + (size_t)tx] = sum / (float)(nx * ny);
    }
}

// k_resolve with spp read per pixel from its tile's entry: the same inv, the same
// (0.0f + acc) * inv, radiance and BGRA written the same way.  The whole frame.
__global__ void k_resolve_tiles(ResolveTilesArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t npix = (size_t)a.width * (size_t)a.height;
    const size_t off = (size_t)x + (size_t)y * (size_t)a.width;
    const int spp = a.tile_spp[(size_t)(y >> 4) * (size_t)a.tiles_x + (size_t)(x >> 4)];
    const float inv = 1.0f / (float)spp;
    const float r = (0.0f + a.accum[off]) * inv;
    const float g = (0.0f + a.accum[npix + off]) * inv;
    const float b = (0.0f + a.accum[2 * npix + off]) * inv;
    if (a.radiance) {
        a.radiance[3 * off] = r;
        a.radiance[3 * off + 1] = g;
        a.radiance[3 * off + 2] = b;
    }
    if (a.bgra) {   // Spectrum::toUChar, as k_resolve
        uint8_t* px = a.bgra + 4 * ((size_t)(a.height - y - 1) * (size_t)a.width + (size_t)x);
        px[0] = to_uchar(b);
        px[1] = to_uchar(g);
        px[2] = to_uchar(r);
    }
}

hipError_t launch_tile_error(const TileErrorArgs& a, hipStream_t s) {
    if (a.n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tile_error, dim3((unsigned)a.n_tiles), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_resolve_tiles(const ResolveTilesArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_resolve_tiles, dim3((a.width + 255) / 256, a.height), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace tpt
