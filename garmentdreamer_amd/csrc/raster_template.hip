// raster_template.hip -- fixed-radius nearest-sample search on a uniform grid (C-ABI: include/gd_scene.h,
// gd_scene_shell_*): the "shell" step of the garment-template initialisation.
//
// Reference: GaussianDreamer.add_points (Garment_3DGS/threestudio/systems/GaussianDreamer.py:115-144) asks a KD-tree for
// the nearest of the 50 000 template samples of each of 500 000 box-uniform candidates, one Python iteration per
// candidate, and keeps the candidate when that sample is closer than `deviation`.  Only candidates with a sample inside
// the radius matter, so a uniform grid with a cell edge >= radius answers the same question from the cells next to
// the query.
//
//   count    one atomic per sample into its cell's counter
//   scan     exclusive prefix over the cells: 1024 cells per workgroup, the workgroup totals through
//            launch_scan_block_sums (raster_binning.hip)
//   scatter  pos = atomicAdd(cell, 1): the counter array ends up holding each cell's END, the samples sit in cell
//            order as packed float4 {x, y, z, bits of the original index}: one 16-byte load per candidate
//   search   one thread per query.  Cells are numbered x-fastest, so the cells lo_x..hi_x of one (y, z) row are ONE
//            contiguous span of the packed array: 9 spans (18 loads of the end array) instead of 27 cell lists.
//
// Result rules (the host test states them again in numpy):
//   d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), fp32, this file is built with -ffp-contract=off;
//   smallest d2 wins, on equal d2 the LOWEST sample index: the order atomics leave inside a cell does not matter and
//   reruns are bit-identical;  nearest = index if d2 < fl(radius radius) else -1;  dist2 = the minimum over the
//   visited cells (+inf when they were empty).
//
// Which cells a query visits.  cell(p) = clamp(floor(fl(fl(p - min) / edge))) is monotone in p, and a sample the
// fp32 test above can accept lies within reach = radius (1 + 1e-6) of the query on every axis (the six roundings of
// d2 and the one of radius^2 move the decision by < 2e-7 relative).  Rounding is monotone too, so
// cell(fl(q - reach)) <= cell(s) <= cell(fl(q + reach)): that range is what the kernel walks.  With edge >= radius it
// is the query's cell and its neighbours (3 per axis, 27 in all) except for a query within 1e-6 edge of a cell face,
// where it can be 4 on that axis -- never too few, which a fixed "own cell +- 1" would be in that same case.
#include <float.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gd_scene.h"
#include "raster_common.h"

namespace gd {

namespace {

constexpr int kAxisCells = GD_SCENE_SHELL_AXIS_CELLS;   // extent / edge <= 255 -> at most 256 cells per axis, 2^24 in all
constexpr int kScanTile = 1024;                         // cells per workgroup of the prefix sum (256 threads x uint4)

struct ShellGrid {
    float mn[3];
    float edge;
    int dim[3];
    float r2;      // fl(radius * radius)
    float reach;   // radius * (1 + 1e-6): see the header comment
};

// nullptr, or what is wrong with the arguments
const char* plan_grid(const float* bbox_min, const float* bbox_max, float radius, ShellGrid* g)
{
    if (!bbox_min || !bbox_max) return "shell: null bounding box";
    if (!(radius > 0.0f) || !(radius <= FLT_MAX)) return "shell: radius must be positive and finite";
    float longest = 0.0f;
    for (int k = 0; k < 3; k++) {
        const float ext = bbox_max[k] - bbox_min[k];
        if (!(ext >= 0.0f) || !(ext <= FLT_MAX) || !(fabsf(bbox_min[k]) <= FLT_MAX))
            return "shell: bounding box must be finite with max >= min";
        longest = fmaxf(longest, ext);
    }
    g->edge = fmaxf(radius, longest / (float)kAxisCells);
    for (int k = 0; k < 3; k++) {
        g->mn[k] = bbox_min[k];
        const float cells = floorf((bbox_max[k] - bbox_min[k]) / g->edge) + 1.0f;
        g->dim[k] = (int)fminf(fmaxf(cells, 1.0f), (float)(kAxisCells + 1));
    }
    g->r2 = radius * radius;
    g->reach = radius * 1.000001f;
    return nullptr;
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct ShellScratch {
    uint32_t* cells;        // [ntiles * kScanTile] counts -> starts -> ends
    uint32_t* tile_sums;    // [ntiles + 1]
    float4* packed;         // [S]
    size_t ntiles, total;
};

ShellScratch carve_shell(char* base, int S, int64_t cells)
{
    ShellScratch c;
    size_t off = 0;
    c.ntiles = ((size_t)cells + kScanTile - 1) / kScanTile;
    c.cells = (uint32_t*)(base + off); off = align_up(off + c.ntiles * kScanTile * sizeof(uint32_t));
    c.tile_sums = (uint32_t*)(base + off); off = align_up(off + (c.ntiles + 1) * sizeof(uint32_t));
    c.packed = (float4*)(base + off); off = align_up(off + (size_t)(S > 0 ? S : 0) * sizeof(float4));
    c.total = off;
    return c;
}

__device__ __forceinline__ float cell_coord(float p, float mn, float edge) { return floorf((p - mn) / edge); }

__device__ __forceinline__ int sample_cell(const ShellGrid& g, float x, float y, float z)
{
    const int cx = (int)fminf(fmaxf(cell_coord(x, g.mn[0], g.edge), 0.0f), (float)(g.dim[0] - 1));
    const int cy = (int)fminf(fmaxf(cell_coord(y, g.mn[1], g.edge), 0.0f), (float)(g.dim[1] - 1));
    const int cz = (int)fminf(fmaxf(cell_coord(z, g.mn[2], g.edge), 0.0f), (float)(g.dim[2] - 1));
    return (cz * g.dim[1] + cy) * g.dim[0] + cx;
}

__global__ __launch_bounds__(256) void shell_count_kernel(int S, const float* __restrict__ samples, ShellGrid g,
                                                          uint32_t* __restrict__ cells)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    atomicAdd(&cells[sample_cell(g, samples[3 * (size_t)i], samples[3 * (size_t)i + 1], samples[3 * (size_t)i + 2])], 1u);
}

__global__ __launch_bounds__(256) void shell_tile_sum_kernel(const uint32_t* __restrict__ cells,
                                                             uint32_t* __restrict__ tile_sums)
{
    __shared__ uint32_t s_wave[4];
    const uint4 v = reinterpret_cast<const uint4*>(cells)[(size_t)blockIdx.x * 256 + threadIdx.x];
    uint32_t sum = v.x + v.y + v.z + v.w;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// counts -> exclusive starts, in place; tile_sums holds the exclusive scan of the workgroup totals by now
__global__ __launch_bounds__(256) void shell_tile_scan_kernel(uint32_t* __restrict__ cells,
                                                              const uint32_t* __restrict__ tile_sums)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4* p = reinterpret_cast<uint4*>(cells) + (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint4 v = *p;
    const uint32_t sum = v.x + v.y + v.z + v.w;
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t e = tile_sums[blockIdx.x] + incl - sum;
    for (uint32_t w = 0; w < wave; w++) e += s_wave[w];
    *p = make_uint4(e, e + v.x, e + v.x + v.y, e + v.x + v.y + v.z);
}

// cells[c] is the next free position of cell c; when every sample is placed it is the cell's end
__global__ __launch_bounds__(256) void shell_scatter_kernel(int S, const float* __restrict__ samples, ShellGrid g,
                                                            uint32_t* __restrict__ cells, float4* __restrict__ packed)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const float x = samples[3 * (size_t)i], y = samples[3 * (size_t)i + 1], z = samples[3 * (size_t)i + 2];
    const uint32_t pos = atomicAdd(&cells[sample_cell(g, x, y, z)], 1u);
    if (pos < (uint32_t)S) packed[pos] = make_float4(x, y, z, __int_as_float(i));
}

__global__ __launch_bounds__(256) void shell_search_kernel(int Q, const float* __restrict__ queries, ShellGrid g,
                                                           const uint32_t* __restrict__ cell_end,
                                                           const float4* __restrict__ packed, int* __restrict__ nearest,
                                                           float* __restrict__ dist2)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const float qp[3] = {queries[3 * (size_t)q], queries[3 * (size_t)q + 1], queries[3 * (size_t)q + 2]};
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {   // cells past the grid are skipped: lo may be dim, hi may be -1 (NaN: empty too)
        lo[k] = (int)fminf(fmaxf(cell_coord(qp[k] - g.reach, g.mn[k], g.edge), 0.0f), (float)g.dim[k]);
        hi[k] = (int)fminf(fmaxf(cell_coord(qp[k] + g.reach, g.mn[k], g.edge), -1.0f), (float)(g.dim[k] - 1));
    }
    float best = INFINITY;
    int best_i = INT_MAX;
    if (lo[0] <= hi[0]) {
        for (int cz = lo[2]; cz <= hi[2]; cz++) {
            for (int cy = lo[1]; cy <= hi[1]; cy++) {
                const int row = (cz * g.dim[1] + cy) * g.dim[0];
                const int first = row + lo[0];
                uint32_t j = first > 0 ? cell_end[first - 1] : 0u;
                const uint32_t end = cell_end[row + hi[0]];
                for (; j < end; j++) {
                    const float4 c = packed[j];
                    const float dx = c.x - qp[0], dy = c.y - qp[1], dz = c.z - qp[2];
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const int idx = __float_as_int(c.w);
                    if (d2 < best || (d2 == best && idx < best_i)) {
                        best = d2;
                        best_i = idx;
                    }
                }
            }
        }
    }
    nearest[q] = best < g.r2 ? best_i : -1;
    dist2[q] = best;
}

}  // namespace
}  // namespace gd

extern "C" {

int gd_scene_shell_grid(const float* bbox_min, const float* bbox_max, float radius, float* cell_edge, int* dims)
{
    using namespace gd;
    ShellGrid g;
    if (const char* err = plan_grid(bbox_min, bbox_max, radius, &g)) return scene_fail(-1, err);
    if (!cell_edge || !dims) return scene_fail(-1, "shell: null output pointer");
    *cell_edge = g.edge;
    for (int k = 0; k < 3; k++) dims[k] = g.dim[k];
    return 0;
}

size_t gd_scene_shell_scratch_bytes(int S, int64_t cells)
{
    if (cells < 1) cells = 1;
    return gd::carve_shell(nullptr, S, cells).total;
}

int gd_scene_shell_search(void* stream, int S, const float* samples, int Q, const float* queries, const float* bbox_min,
                          const float* bbox_max, float radius, int* nearest, float* dist2, void* scratch)
{
    using namespace gd;
    if (S < 0) return scene_fail(-1, "shell: S must be >= 0");
    if (Q < 0) return scene_fail(-1, "shell: Q must be >= 0");
    ShellGrid g;
    if (const char* err = plan_grid(bbox_min, bbox_max, radius, &g)) return scene_fail(-1, err);
    if (Q == 0) return 0;
    if ((S > 0 && !samples) || !queries || !nearest || !dist2 || !scratch) return scene_fail(-1, "shell: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t cells = (int64_t)g.dim[0] * g.dim[1] * g.dim[2];
    ShellScratch c = carve_shell((char*)scratch, S, cells);
    hipError_t e = hipMemsetAsync(c.cells, 0, c.ntiles * kScanTile * sizeof(uint32_t), s);
    if (e != hipSuccess) return scene_fail(-2, hipGetErrorString(e));
    const int sblk = (S + 255) / 256;
    if (S > 0) hipLaunchKernelGGL(shell_count_kernel, dim3(sblk), dim3(256), 0, s, S, samples, g, c.cells);
    hipLaunchKernelGGL(shell_tile_sum_kernel, dim3((unsigned)c.ntiles), dim3(256), 0, s, c.cells, c.tile_sums);
    launch_scan_block_sums(s, c.tile_sums, (uint32_t)c.ntiles);
    hipLaunchKernelGGL(shell_tile_scan_kernel, dim3((unsigned)c.ntiles), dim3(256), 0, s, c.cells, c.tile_sums);
    if (S > 0) hipLaunchKernelGGL(shell_scatter_kernel, dim3(sblk), dim3(256), 0, s, S, samples, g, c.cells, c.packed);
    hipLaunchKernelGGL(shell_search_kernel, dim3((Q + 255) / 256), dim3(256), 0, s, Q, queries, g, c.cells, c.packed,
                       nearest, dist2);
    e = hipGetLastError();
    if (e != hipSuccess) return scene_fail(-2, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
