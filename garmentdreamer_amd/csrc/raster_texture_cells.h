// raster_texture_cells.h -- the cell arithmetic of the hash-grid encoding (DEFINITIONS: include/gd_texture.h), shared by
// raster_texture.hip and raster_texture_sorted.hip so that both form the same indices and weights bit for bit, and the host
// interface between the two files.  Every file that includes this is built with -ffp-contract=off.
#ifndef GD_RASTER_TEXTURE_CELLS_H_INCLUDED
#define GD_RASTER_TEXTURE_CELLS_H_INCLUDED

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gd_texture.h"

namespace gd {
namespace {

struct Level {
    float scale;
    uint32_t res, size, offset;
    bool dense, pow2;
};

__device__ __forceinline__ Level level_of(const gd_texture_layout& lay, int l)
{
    Level v;
    v.scale = lay.scale[l];
    v.res = (uint32_t)lay.res[l];
    v.size = (uint32_t)lay.size[l];
    v.offset = (uint32_t)lay.offset[l];
    v.dense = (uint64_t)v.res * v.res * v.res <= (uint64_t)v.size;
    v.pow2 = (v.size & (v.size - 1)) == 0;
    return v;
}

struct Cell {
    uint32_t c[3];
    float w[3];
};

__device__ __forceinline__ Cell cell_of(const float u[3], float scale)
{
    Cell ce;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        float p = scale * u[d];
        p = p + 0.5f;
        const float fl = floorf(p);
        ce.c[d] = (uint32_t)(int32_t)fl;
        ce.w[d] = p - fl;
    }
    return ce;
}

// always < lv.size
__device__ __forceinline__ uint32_t corner_index(const Level& lv, const Cell& ce, int i)
{
    const uint32_t g0 = ce.c[0] + (uint32_t)(i & 1), g1 = ce.c[1] + (uint32_t)((i >> 1) & 1),
                   g2 = ce.c[2] + (uint32_t)((i >> 2) & 1);
    const uint32_t idx = lv.dense ? g0 + g1 * lv.res + g2 * lv.res * lv.res
                                  : g0 ^ (g1 * 2654435761u) ^ (g2 * 805459861u);
    if (lv.pow2) return idx & (lv.size - 1);
    return idx < lv.size ? idx : idx % lv.size;
}

__device__ __forceinline__ float corner_weight(const Cell& ce, int i)
{
    const float a = (i & 1) ? ce.w[0] : 1.0f - ce.w[0];
    const float b = (i & 2) ? ce.w[1] : 1.0f - ce.w[1];
    const float c = (i & 4) ? ce.w[2] : 1.0f - ce.w[2];
    return (a * b) * c;
}

// the point's u, or false for a point that takes no part (beyond N, masked out, or a non-finite coordinate)
__device__ __forceinline__ bool load_point(int n, int N, const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                           float u[3])
{
    if (n >= N) return false;
    if (mask && mask[n] == 0) return false;
    const float x0 = x[3 * (size_t)n], x1 = x[3 * (size_t)n + 1], x2 = x[3 * (size_t)n + 2];
    if (!(__builtin_isfinite(x0) && __builtin_isfinite(x1) && __builtin_isfinite(x2))) return false;
    u[0] = (x0 + 1.0f) * 0.5f;
    u[1] = (x1 + 1.0f) * 0.5f;
    u[2] = (x2 + 1.0f) * 0.5f;
    return true;
}

}  // namespace

// raster_texture_sorted.hip: dgrid by stable sort and sum (include/gd_texture_sorted.h).  The layout is consistent and
// 1 <= N <= 2^24 (the entries of raster_texture.hip check both); only launches, no HIP call that waits.
constexpr int kSortedMaxPoints = 1 << 24;
size_t sorted_dgrid_scratch_bytes(int N, const gd_texture_layout& lay);
void launch_sorted_dgrid(hipStream_t s, int N, const float* x, const uint8_t* mask, const float* denc,
                         const gd_texture_layout& lay, float* dgrid, void* scratch);

}  // namespace gd
#endif
