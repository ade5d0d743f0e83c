// raster_texture.hip -- the NeTF stage's texture field (C-ABI and the DEFINITIONS: include/gd_texture.h): the
// multiresolution hash-grid encoding of tiny-cuda-nn's "Grid"/"Hash" with linear interpolation, and the fused
// color = sigmoid(mlp(encode(x))) of Garment_Deformer_NeTF/netf/render/mesh_renderer.py:368-375, forward and backward.
// Built with -ffp-contract=off: the header fixes the order of every operation of the encoding (the tests compare it bit
// for bit with an fp32 numpy statement).  The MLP's products are written as explicit fmaf.
//
//   encode forward / backward   one thread per point, the levels in a loop; forward gathers 8 float2 per level, backward
//                               scatters 8 x 2 no-return fp32 atomicAdd per level
//   field forward               one thread per point, 256 per workgroup; the 1 155 MLP floats in LDS, read at one address
//                               by the whole wave (a broadcast); the 32 encoded features never leave the registers
//   field backward              128 points per workgroup pass.  Each thread recomputes enc and h of its point, forms denc
//                               = W1^T dh in registers and scatters it; enc, h and do go to LDS, and after a barrier the
//                               workgroup adds the 1 155 weight-gradient terms over its points in ascending order, each
//                               thread owning 8 entries of dW1 (and up to three of the small ones).  A workgroup walks
//                               chunks blockIdx, blockIdx + gridDim, ... and keeps its sums in registers; it writes ONE
//                               slab row at the end.  slab_sum_kernel adds the rows in ascending order to the
//                               destinations: no float atomics on the MLP gradients, reruns bit-identical.
//   dgrid                       plain atomics; its last bits depend on arrival order (stated in the header).  The opt-in
//                               reproducible form (include/gd_texture_sorted.h) has its entries here and its kernels in
//                               raster_texture_sorted.hip; its fused variant is field_backward_kernel<true>, which stores
//                               denc [N][32] instead of scattering it.
//   dx                          the opt-in gradient to the positions (include/gd_texture_position.h): position_level gathers
//                               each corner once; alone in encode_backward_pos_kernel, or in field_backward_pos_kernel beside
//                               the scatter (or the store of denc), the levels in a rolled loop with denc in LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_texture.h"
#include "../../include/gd_texture_sorted.h"
#include "../../include/gd_texture_position.h"
#include "raster_texture_cells.h"

namespace gd {
namespace {

thread_local char g_texture_err[256] = "";

int tfail(int code, const char* msg)
{
    snprintf(g_texture_err, sizeof(g_texture_err), "%s", msg);
    return code;
}

constexpr int kLevels = GD_TEXTURE_MAX_LEVELS;
constexpr int kWidth = GD_TEXTURE_FIELD_WIDTH;
constexpr int kW1 = 0, kB1 = kWidth * kWidth, kW2 = kB1 + kWidth, kB2 = kW2 + 3 * kWidth;   // offsets in the MLP block
constexpr int kMlpFloats = kB2 + 3;                                                          // 1155
constexpr int kSlabRow = 1156;
constexpr int kBwdThreads = 128;      // points per pass of a backward workgroup
constexpr int kRowStride = 36;        // floats per point in the LDS images of enc and h: rows stay 16-byte aligned
constexpr int kMaxSlabRows = 1024;
constexpr int kDencStride = 33;       // floats per point in the LDS image of denc (field_backward_pos_kernel): odd, no conflicts
constexpr int kSumCols = 16, kSumGroups = 16;

__device__ __forceinline__ float2 encode_level(const float2* __restrict__ grid, const Level& lv, const float u[3])
{
    const Cell ce = cell_of(u, lv.scale);
    float2 acc = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const float2 g = grid[(size_t)lv.offset + corner_index(lv, ce, i)];
        const float w = corner_weight(ce, i);
        acc.x = acc.x + w * g.x;
        acc.y = acc.y + w * g.y;
    }
    return acc;
}

__device__ __forceinline__ void scatter_level(float* __restrict__ dgrid, const Level& lv, const float u[3], float d0,
                                              float d1)
{
    const Cell ce = cell_of(u, lv.scale);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        float* dst = dgrid + ((size_t)lv.offset + corner_index(lv, ce, i)) * GD_TEXTURE_FEATURES;
        const float w = corner_weight(ce, i);
        atomicAdd(dst, w * d0);
        atomicAdd(dst + 1, w * d1);
    }
}

// One level of the gradient to the position (DEFINITION: include/gd_texture_position.h): S_d over the eight corners, each
// grid entry gathered once; with kScatter the corner's dgrid contribution is added in the same step, the two atomics being
// those of scatter_level bit for bit.  Returns with dx_d = dx_d + (0.5 s_l) S_d.
template <bool kScatter>
__device__ __forceinline__ void position_level(const float2* __restrict__ grid, float* __restrict__ dgrid, const Level& lv,
                                               const float u[3], float d0, float d1, float dx[3])
{
    const Cell ce = cell_of(u, lv.scale);
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const size_t e = (size_t)lv.offset + corner_index(lv, ce, i);
        const float2 g = grid[e];
        const float a = (i & 1) ? ce.w[0] : 1.0f - ce.w[0];
        const float b = (i & 2) ? ce.w[1] : 1.0f - ce.w[1];
        const float c = (i & 4) ? ce.w[2] : 1.0f - ce.w[2];
        if constexpr (kScatter) {
            const float w = (a * b) * c;          // corner_weight
            atomicAdd(dgrid + e * GD_TEXTURE_FEATURES, w * d0);
            atomicAdd(dgrid + e * GD_TEXTURE_FEATURES + 1, w * d1);
        }
        const float t = d0 * g.x + d1 * g.y;
        const float q0 = (b * c) * t, q1 = (a * c) * t, q2 = (a * b) * t;
        s0 = (i & 1) ? s0 + q0 : s0 - q0;
        s1 = (i & 2) ? s1 + q1 : s1 - q1;
        s2 = (i & 4) ? s2 + q2 : s2 - q2;
    }
    const float k = 0.5f * lv.scale;
    dx[0] = dx[0] + k * s0;
    dx[1] = dx[1] + k * s1;
    dx[2] = dx[2] + k * s2;
}

// ---- the encoding on its own ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void encode_forward_kernel(int N, const float* __restrict__ x,
                                                             const uint8_t* __restrict__ mask,
                                                             const float2* __restrict__ grid, gd_texture_layout lay,
                                                             float* __restrict__ enc)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float u[3];
    const bool valid = load_point(n, N, x, mask, u);
    float* out = enc + (size_t)n * lay.num_levels * GD_TEXTURE_FEATURES;
    for (int l = 0; l < lay.num_levels; l++) {
        float2 e = make_float2(0.0f, 0.0f);
        if (valid) e = encode_level(grid, level_of(lay, l), u);
        out[2 * l] = e.x;
        out[2 * l + 1] = e.y;
    }
}

__global__ __launch_bounds__(256) void encode_backward_kernel(int N, const float* __restrict__ x,
                                                              const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ denc, gd_texture_layout lay,
                                                              float* __restrict__ dgrid)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    float u[3];
    if (!load_point(n, N, x, mask, u)) return;
    const float* d = denc + (size_t)n * lay.num_levels * GD_TEXTURE_FEATURES;
    for (int l = 0; l < lay.num_levels; l++) {
        scatter_level(dgrid, level_of(lay, l), u, d[2 * l], d[2 * l + 1]);
    }
}

// dx [N][3], every row written
__global__ __launch_bounds__(256) void encode_backward_pos_kernel(int N, const float* __restrict__ x,
                                                                  const uint8_t* __restrict__ mask,
                                                                  const float2* __restrict__ grid, gd_texture_layout lay,
                                                                  const float* __restrict__ denc, float* __restrict__ dx)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float u[3];
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (load_point(n, N, x, mask, u)) {
        const float* d = denc + (size_t)n * lay.num_levels * GD_TEXTURE_FEATURES;
        for (int l = 0; l < lay.num_levels; l++)
            position_level<false>(grid, nullptr, level_of(lay, l), u, d[2 * l], d[2 * l + 1], acc);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) dx[3 * (size_t)n + c] = acc[c];
}

// ---- the fused field -----------------------------------------------------------------------------------------------------

__device__ __forceinline__ void load_mlp(float* mlp, const float* __restrict__ w1, const float* __restrict__ b1,
                                         const float* __restrict__ w2, const float* __restrict__ b2)
{
    for (int i = threadIdx.x; i < kWidth * kWidth; i += blockDim.x) mlp[kW1 + i] = w1[i];
    for (int i = threadIdx.x; i < kWidth; i += blockDim.x) mlp[kB1 + i] = b1[i];
    for (int i = threadIdx.x; i < 3 * kWidth; i += blockDim.x) mlp[kW2 + i] = w2[i];
    for (int i = threadIdx.x; i < 3; i += blockDim.x) mlp[kB2 + i] = b2[i];
}

__device__ __forceinline__ void encode_all(const float2* __restrict__ grid, const gd_texture_layout& lay,
                                           const float u[3], float enc[kWidth])
{
#pragma unroll
    for (int l = 0; l < kLevels; l++) {
        const float2 e = encode_level(grid, level_of(lay, l), u);
        enc[2 * l] = e.x;
        enc[2 * l + 1] = e.y;
    }
}

// z_j = b1[j] + sum_k W1[j][k] enc[k], ascending k
__device__ __forceinline__ float hidden_preact(const float* mlp, int j, const float enc[kWidth])
{
    float z = mlp[kB1 + j];
#pragma unroll
    for (int k = 0; k < kWidth; k++) z = __builtin_fmaf(mlp[kW1 + j * kWidth + k], enc[k], z);
    return z;
}

// dh_j = [h_j > 0] (W2^T do)_j
__device__ __forceinline__ float hidden_grad(float h, float w20, float w21, float w22, float d0, float d1, float d2)
{
    const float g = __builtin_fmaf(w22, d2, __builtin_fmaf(w21, d1, w20 * d0));
    return h > 0.0f ? g : 0.0f;
}

__global__ __launch_bounds__(256) void field_forward_kernel(int N, const float* __restrict__ x,
                                                            const uint8_t* __restrict__ mask,
                                                            const float2* __restrict__ grid, gd_texture_layout lay,
                                                            const float* __restrict__ w1, const float* __restrict__ b1,
                                                            const float* __restrict__ w2, const float* __restrict__ b2,
                                                            float* __restrict__ color)
{
    __shared__ float mlp[kSlabRow];
    load_mlp(mlp, w1, b1, w2, b2);
    __syncthreads();
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float u[3];
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (load_point(n, N, x, mask, u)) {
        float enc[kWidth];
        encode_all(grid, lay, u, enc);
        float a[3] = {mlp[kB2], mlp[kB2 + 1], mlp[kB2 + 2]};
        for (int j = 0; j < kWidth; j++) {
            const float h = fmaxf(hidden_preact(mlp, j, enc), 0.0f);
#pragma unroll
            for (int c = 0; c < 3; c++) a[c] = __builtin_fmaf(mlp[kW2 + c * kWidth + j], h, a[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) o[c] = 1.0f / (1.0f + expf(-a[c]));
    }
#pragma unroll
    for (int c = 0; c < 3; c++) color[3 * (size_t)n + c] = o[c];
}

// kStoreDenc = false: denc is scattered into dgrid with atomics.  kStoreDenc = true (the sorted path): dgrid is not touched
// and the point's row of denc [N][32] is stored instead, zeros for a point that takes no part; the same parameter carries
// either pointer, so that the atomic instantiation keeps its signature and its code.
//
// kPosGrad (include/gd_texture_position.h): dx [N][3] is written beside it, every row; the levels then go through
// position_level, which gathers each corner's grid entry where its contribution is (or, on the sorted path, would be)
// scattered.  The body is shared; the kernels without dx keep their signatures.
template <bool kStoreDenc, bool kPosGrad>
__device__ __forceinline__ void field_backward_body(
    int N, int nchunks, const float* __restrict__ x, const uint8_t* __restrict__ mask, const float2* __restrict__ grid,
    const gd_texture_layout& lay, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ color,
    const float* __restrict__ dcolor, float* __restrict__ dgrid, float* __restrict__ slab, float* __restrict__ dx)
{
    __shared__ float mlp[kSlabRow];
    __shared__ __align__(16) float encS[kBwdThreads * kRowStride];
    __shared__ __align__(16) float hS[kBwdThreads * kRowStride];
    __shared__ float4 doS[kBwdThreads];
    load_mlp(mlp, w1, b1, w2, b2);

    const int t = threadIdx.x;
    // this thread's entries of the weight gradients: dW1[jw][kw .. kw + 7]; db1[jw] where kw == 0; dW2 entry t (row t / 32,
    // column t % 32) for t < 96; db2[t] for t < 3
    const int jw = t >> 2, kw = (t & 3) * 8;
    float aw1[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float ab1 = 0.0f, aw2 = 0.0f, ab2 = 0.0f;

    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        __syncthreads();   // the MLP block is loaded; the previous pass has read enc / h / do
        const int n = chunk * kBwdThreads + t;
        float u[3];
        const bool valid = load_point(n, N, x, mask, u);
        float enc[kWidth];
        float d[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < kWidth; k++) enc[k] = 0.0f;
        if (valid) {
            encode_all(grid, lay, u, enc);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float col = color[3 * (size_t)n + c];
                d[c] = (dcolor[3 * (size_t)n + c] * col) * (1.0f - col);
            }
        }
#pragma unroll
        for (int k = 0; k < kWidth; k++) encS[t * kRowStride + k] = enc[k];
        doS[t] = make_float4(d[0], d[1], d[2], 0.0f);
        if (valid) {
            float denc[kWidth];
#pragma unroll
            for (int k = 0; k < kWidth; k++) denc[k] = 0.0f;
            for (int j = 0; j < kWidth; j++) {
                const float h = fmaxf(hidden_preact(mlp, j, enc), 0.0f);
                hS[t * kRowStride + j] = h;
                const float dh = hidden_grad(h, mlp[kW2 + j], mlp[kW2 + kWidth + j], mlp[kW2 + 2 * kWidth + j], d[0],
                                             d[1], d[2]);
#pragma unroll
                for (int k = 0; k < kWidth; k++) denc[k] = __builtin_fmaf(mlp[kW1 + j * kWidth + k], dh, denc[k]);
            }
            if constexpr (kStoreDenc) {
                float4* row = reinterpret_cast<float4*>(dgrid + (size_t)n * kWidth);
#pragma unroll
                for (int k = 0; k < kWidth / 4; k++)
                    row[k] = make_float4(denc[4 * k], denc[4 * k + 1], denc[4 * k + 2], denc[4 * k + 3]);
            } else if constexpr (!kPosGrad) {
#pragma unroll
                for (int l = 0; l < kLevels; l++) scatter_level(dgrid, level_of(lay, l), u, denc[2 * l], denc[2 * l + 1]);
            }
            if constexpr (kPosGrad) {
                // the levels in a ROLLED loop, denc read back from the thread's own LDS row: unrolled over the 16 levels the
                // compiler forms all 128 corner addresses and weights ahead of the gathers and the atomic instantiation
                // spills (172 bytes a lane on top of 256 + 256 registers)
                __shared__ float dencS[kBwdThreads * kDencStride];
#pragma unroll
                for (int k = 0; k < kWidth; k++) dencS[t * kDencStride + k] = denc[k];
                float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
                for (int l = 0; l < kLevels; l++)
                    position_level<!kStoreDenc>(grid, dgrid, level_of(lay, l), u, dencS[t * kDencStride + 2 * l],
                                                dencS[t * kDencStride + 2 * l + 1], acc);
#pragma unroll
                for (int c = 0; c < 3; c++) dx[3 * (size_t)n + c] = acc[c];
            }
        } else {
            for (int j = 0; j < kWidth; j++) hS[t * kRowStride + j] = 0.0f;
            if constexpr (kPosGrad) {
                if (n < N) {
#pragma unroll
                    for (int c = 0; c < 3; c++) dx[3 * (size_t)n + c] = 0.0f;
                }
            }
            if constexpr (kStoreDenc) {
                if (n < N) {
                    float4* row = reinterpret_cast<float4*>(dgrid + (size_t)n * kWidth);
#pragma unroll
                    for (int k = 0; k < kWidth / 4; k++) row[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
            }
        }
        __syncthreads();

        // the weight gradients of this pass, its points in ascending order
        const float w20 = mlp[kW2 + jw], w21 = mlp[kW2 + kWidth + jw], w22 = mlp[kW2 + 2 * kWidth + jw];
        for (int p = 0; p < kBwdThreads; p++) {
            const float4 dp = doS[p];
            const float dh = hidden_grad(hS[p * kRowStride + jw], w20, w21, w22, dp.x, dp.y, dp.z);
            const float4 e0 = *reinterpret_cast<const float4*>(&encS[p * kRowStride + kw]);
            const float4 e1 = *reinterpret_cast<const float4*>(&encS[p * kRowStride + kw + 4]);
            aw1[0] = __builtin_fmaf(dh, e0.x, aw1[0]);
            aw1[1] = __builtin_fmaf(dh, e0.y, aw1[1]);
            aw1[2] = __builtin_fmaf(dh, e0.z, aw1[2]);
            aw1[3] = __builtin_fmaf(dh, e0.w, aw1[3]);
            aw1[4] = __builtin_fmaf(dh, e1.x, aw1[4]);
            aw1[5] = __builtin_fmaf(dh, e1.y, aw1[5]);
            aw1[6] = __builtin_fmaf(dh, e1.z, aw1[6]);
            aw1[7] = __builtin_fmaf(dh, e1.w, aw1[7]);
            ab1 = ab1 + dh;
        }
        if (t < 3 * kWidth) {
            const int c = t >> 5, j = t & 31;
            const float* dcomp = reinterpret_cast<const float*>(doS) + c;
            for (int p = 0; p < kBwdThreads; p++) aw2 = __builtin_fmaf(dcomp[4 * p], hS[p * kRowStride + j], aw2);
        }
        if (t < 3) {
            const float* dcomp = reinterpret_cast<const float*>(doS) + t;
            for (int p = 0; p < kBwdThreads; p++) ab2 = ab2 + dcomp[4 * p];
        }
    }

    float* row = slab + (size_t)blockIdx.x * kSlabRow;
#pragma unroll
    for (int i = 0; i < 8; i++) row[kW1 + jw * kWidth + kw + i] = aw1[i];
    if (kw == 0) row[kB1 + jw] = ab1;
    if (t < 3 * kWidth) row[kW2 + t] = aw2;
    if (t < 3) row[kB2 + t] = ab2;
}

template <bool kStoreDenc>
__global__ __launch_bounds__(kBwdThreads) void field_backward_kernel(
    int N, int nchunks, const float* __restrict__ x, const uint8_t* __restrict__ mask, const float2* __restrict__ grid,
    gd_texture_layout lay, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ color, const float* __restrict__ dcolor,
    float* __restrict__ dgrid, float* __restrict__ slab)
{
    field_backward_body<kStoreDenc, false>(N, nchunks, x, mask, grid, lay, w1, b1, w2, b2, color, dcolor, dgrid, slab,
                                           nullptr);
}

template <bool kStoreDenc>
__global__ __launch_bounds__(kBwdThreads) void field_backward_pos_kernel(
    int N, int nchunks, const float* __restrict__ x, const uint8_t* __restrict__ mask, const float2* __restrict__ grid,
    gd_texture_layout lay, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ color, const float* __restrict__ dcolor,
    float* __restrict__ dgrid, float* __restrict__ slab, float* __restrict__ dx)
{
    field_backward_body<kStoreDenc, true>(N, nchunks, x, mask, grid, lay, w1, b1, w2, b2, color, dcolor, dgrid, slab, dx);
}

// dst[e] += sum of the slab's rows, ascending: thread (column, group) adds rows group, group + 16, ... from 0, then the 16
// groups of a column are added in ascending order from 0
__global__ __launch_bounds__(kSumCols* kSumGroups) void slab_sum_kernel(int rows, const float* __restrict__ slab,
                                                                        float* __restrict__ dw1, float* __restrict__ db1,
                                                                        float* __restrict__ dw2, float* __restrict__ db2)
{
    __shared__ float part[kSumGroups][kSumCols];
    const int c = threadIdx.x % kSumCols, g = threadIdx.x / kSumCols;
    const int e = blockIdx.x * kSumCols + c;
    float s = 0.0f;
    if (e < kMlpFloats)
        for (int r = g; r < rows; r += kSumGroups) s = s + slab[(size_t)r * kSlabRow + e];
    part[g][c] = s;
    __syncthreads();
    if (g != 0 || e >= kMlpFloats) return;
    float total = 0.0f;
#pragma unroll
    for (int i = 0; i < kSumGroups; i++) total = total + part[i][c];
    float* dst = e < kB1 ? dw1 + e : e < kW2 ? db1 + (e - kB1) : e < kB2 ? dw2 + (e - kW2) : db2 + (e - kB2);
    *dst = *dst + total;
}

// ---- host ------------------------------------------------------------------------------------------------------------------

const char* layout_error(const gd_texture_layout& lay)
{
    if (lay.num_levels < 1 || lay.num_levels > kLevels) return "layout: num_levels must be in 1..16";
    if (lay.offset[0] != 0) return "layout: offset[0] must be 0";
    for (int l = 0; l < lay.num_levels; l++) {
        if (lay.res[l] < 1 || lay.res[l] > (1 << 21)) return "layout: res must be in 1..2^21";
        if (lay.size[l] <= 0) return "layout: size must be positive";
        if (lay.offset[l + 1] <= lay.offset[l]) return "layout: offsets must increase";
        if ((int64_t)lay.offset[l + 1] != (int64_t)lay.offset[l] + lay.size[l])
            return "layout: offset[l + 1] must be offset[l] + size[l]";
        if (lay.offset[l + 1] > (1 << 28)) return "layout: more than 2^28 entries";
    }
    return nullptr;
}

int check_common(const char* what, int N, const gd_texture_layout& lay, bool nulls, const void* aligned8)
{
    char buf[200];
    if (N < 0 || N > (1 << 30)) {
        snprintf(buf, sizeof(buf), "%s: N must be in 0..2^30", what);
        return tfail(-1, buf);
    }
    if (nulls) {
        snprintf(buf, sizeof(buf), "%s: null pointer", what);
        return tfail(-1, buf);
    }
    if (const char* e = layout_error(lay)) {
        snprintf(buf, sizeof(buf), "%s: %s", what, e);
        return tfail(-1, buf);
    }
    if (aligned8 && ((uintptr_t)aligned8 & 7)) {
        snprintf(buf, sizeof(buf), "%s: grid must be 8-byte aligned", what);
        return tfail(-1, buf);
    }
    return 0;
}

int need_field_width(const char* what, const gd_texture_layout& lay)
{
    if (lay.num_levels * GD_TEXTURE_FEATURES == kWidth) return 0;
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: the fused field needs num_levels * 2 = 32", what);
    return tfail(-1, buf);
}

int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[200];
        snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
        return tfail(-2, buf);
    }
    return 0;
}

int need_sorted_points(const char* what, int N)
{
    if (N <= kSortedMaxPoints) return 0;
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: N must be in 0..2^24 (item ids and scratch grow with N): use the atomic path or split "
             "the batch", what);
    return tfail(-1, buf);
}

dim3 grid_of(int n, int per) { return dim3((unsigned)(((int64_t)n + per - 1) / per)); }

int backward_chunks(int N) { return (int)(((int64_t)N + kBwdThreads - 1) / kBwdThreads); }
int backward_rows(int N) { return backward_chunks(N) < kMaxSlabRows ? backward_chunks(N) : kMaxSlabRows; }

}  // namespace
}  // namespace gd

extern "C" {

int gd_texture_encode_forward(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                              gd_texture_layout layout, float* enc)
{
    using namespace gd;
    if (int r = check_common("encode forward", N, layout, !x || !grid || !enc, grid)) return r;
    if (N == 0) return 0;
    hipLaunchKernelGGL(encode_forward_kernel, grid_of(N, 256), dim3(256), 0, (hipStream_t)stream, N, x, mask,
                       (const float2*)grid, layout, enc);
    return launched("encode forward");
}

int gd_texture_encode_backward(void* stream, int N, const float* x, const uint8_t* mask, const float* denc,
                               gd_texture_layout layout, float* dgrid)
{
    using namespace gd;
    if (int r = check_common("encode backward", N, layout, !x || !denc || !dgrid, nullptr)) return r;
    if (N == 0) return 0;
    hipLaunchKernelGGL(encode_backward_kernel, grid_of(N, 256), dim3(256), 0, (hipStream_t)stream, N, x, mask, denc,
                       layout, dgrid);
    return launched("encode backward");
}

int gd_texture_field_forward(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                             gd_texture_layout layout, const float* w1, const float* b1, const float* w2,
                             const float* b2, float* color)
{
    using namespace gd;
    if (int r = check_common("field forward", N, layout, !x || !grid || !w1 || !b1 || !w2 || !b2 || !color, grid))
        return r;
    if (int r = need_field_width("field forward", layout)) return r;
    if (N == 0) return 0;
    hipLaunchKernelGGL(field_forward_kernel, grid_of(N, 256), dim3(256), 0, (hipStream_t)stream, N, x, mask,
                       (const float2*)grid, layout, w1, b1, w2, b2, color);
    return launched("field forward");
}

size_t gd_texture_field_backward_scratch_bytes(int N)
{
    if (N <= 0) return 0;
    return ((size_t)gd::backward_rows(N) * gd::kSlabRow * sizeof(float) + 255) & ~(size_t)255;
}

int gd_texture_field_backward(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                              gd_texture_layout layout, const float* w1, const float* b1, const float* w2,
                              const float* b2, const float* color, const float* dcolor, float* dgrid, float* dw1,
                              float* db1, float* dw2, float* db2, void* scratch)
{
    using namespace gd;
    const bool nulls = !x || !grid || !w1 || !b1 || !w2 || !b2 || !color || !dcolor || !dgrid || !dw1 || !db1 || !dw2 ||
                       !db2 || !scratch;
    if (int r = check_common("field backward", N, layout, nulls, grid)) return r;
    if (int r = need_field_width("field backward", layout)) return r;
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int rows = backward_rows(N);
    hipLaunchKernelGGL(field_backward_kernel<false>, dim3((unsigned)rows), dim3(kBwdThreads), 0, s, N, backward_chunks(N),
                       x, mask, (const float2*)grid, layout, w1, b1, w2, b2, color, dcolor, dgrid, (float*)scratch);
    hipLaunchKernelGGL(slab_sum_kernel, grid_of(kMlpFloats, kSumCols), dim3(kSumCols * kSumGroups), 0, s, rows,
                       (const float*)scratch, dw1, db1, dw2, db2);
    return launched("field backward");
}

// ---- dgrid by stable sort and sum (include/gd_texture_sorted.h; the kernels: raster_texture_sorted.hip) --------------------

size_t gd_texture_sorted_scratch_bytes(int N, gd_texture_layout layout)
{
    if (N <= 0 || gd::layout_error(layout)) return 0;      // (defined above 2^24 too: non-decreasing in N)
    return gd::sorted_dgrid_scratch_bytes(N, layout);
}

int gd_texture_encode_backward_sorted(void* stream, int N, const float* x, const uint8_t* mask, const float* denc,
                                      gd_texture_layout layout, float* dgrid, void* scratch)
{
    using namespace gd;
    const char* what = "encode backward sorted";
    if (int r = check_common(what, N, layout, !x || !denc || !dgrid || !scratch, nullptr)) return r;
    if (int r = need_sorted_points(what, N)) return r;
    if (N == 0) return 0;
    launch_sorted_dgrid((hipStream_t)stream, N, x, mask, denc, layout, dgrid, scratch);
    return launched(what);
}

int gd_texture_field_backward_sorted(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                                     gd_texture_layout layout, const float* w1, const float* b1, const float* w2,
                                     const float* b2, const float* color, const float* dcolor, float* dgrid, float* dw1,
                                     float* db1, float* dw2, float* db2, float* denc, void* slab_scratch,
                                     void* sort_scratch)
{
    using namespace gd;
    const char* what = "field backward sorted";
    const bool nulls = !x || !grid || !w1 || !b1 || !w2 || !b2 || !color || !dcolor || !dgrid || !dw1 || !db1 || !dw2 ||
                       !db2 || !denc || !slab_scratch || !sort_scratch;
    if (int r = check_common(what, N, layout, nulls, grid)) return r;
    if (int r = need_field_width(what, layout)) return r;
    if (int r = need_sorted_points(what, N)) return r;
    if ((uintptr_t)denc & 15) return tfail(-1, "field backward sorted: denc must be 16-byte aligned");
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int rows = backward_rows(N);
    hipLaunchKernelGGL(field_backward_kernel<true>, dim3((unsigned)rows), dim3(kBwdThreads), 0, s, N, backward_chunks(N),
                       x, mask, (const float2*)grid, layout, w1, b1, w2, b2, color, dcolor, denc, (float*)slab_scratch);
    hipLaunchKernelGGL(slab_sum_kernel, grid_of(kMlpFloats, kSumCols), dim3(kSumCols * kSumGroups), 0, s, rows,
                       (const float*)slab_scratch, dw1, db1, dw2, db2);
    launch_sorted_dgrid(s, N, x, mask, denc, layout, dgrid, sort_scratch);
    return launched(what);
}

// ---- the gradient to the positions (include/gd_texture_position.h) --------------------------------------------------------

int gd_texture_encode_backward_pos(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                                   gd_texture_layout layout, const float* denc, float* dx)
{
    using namespace gd;
    if (int r = check_common("encode backward pos", N, layout, !x || !grid || !denc || !dx, grid)) return r;
    if (N == 0) return 0;
    hipLaunchKernelGGL(encode_backward_pos_kernel, grid_of(N, 256), dim3(256), 0, (hipStream_t)stream, N, x, mask,
                       (const float2*)grid, layout, denc, dx);
    return launched("encode backward pos");
}

int gd_texture_field_backward_pos(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                                  gd_texture_layout layout, const float* w1, const float* b1, const float* w2,
                                  const float* b2, const float* color, const float* dcolor, float* dgrid, float* dw1,
                                  float* db1, float* dw2, float* db2, float* dx, void* scratch)
{
    using namespace gd;
    const char* what = "field backward pos";
    const bool nulls = !x || !grid || !w1 || !b1 || !w2 || !b2 || !color || !dcolor || !dgrid || !dw1 || !db1 || !dw2 ||
                       !db2 || !dx || !scratch;
    if (int r = check_common(what, N, layout, nulls, grid)) return r;
    if (int r = need_field_width(what, layout)) return r;
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int rows = backward_rows(N);
    hipLaunchKernelGGL(field_backward_pos_kernel<false>, dim3((unsigned)rows), dim3(kBwdThreads), 0, s, N,
                       backward_chunks(N), x, mask, (const float2*)grid, layout, w1, b1, w2, b2, color, dcolor, dgrid,
                       (float*)scratch, dx);
    hipLaunchKernelGGL(slab_sum_kernel, grid_of(kMlpFloats, kSumCols), dim3(kSumCols * kSumGroups), 0, s, rows,
                       (const float*)scratch, dw1, db1, dw2, db2);
    return launched(what);
}

int gd_texture_field_backward_sorted_pos(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                                         gd_texture_layout layout, const float* w1, const float* b1, const float* w2,
                                         const float* b2, const float* color, const float* dcolor, float* dgrid,
                                         float* dw1, float* db1, float* dw2, float* db2, float* denc, float* dx,
                                         void* slab_scratch, void* sort_scratch)
{
    using namespace gd;
    const char* what = "field backward sorted pos";
    const bool nulls = !x || !grid || !w1 || !b1 || !w2 || !b2 || !color || !dcolor || !dgrid || !dw1 || !db1 || !dw2 ||
                       !db2 || !denc || !dx || !slab_scratch || !sort_scratch;
    if (int r = check_common(what, N, layout, nulls, grid)) return r;
    if (int r = need_field_width(what, layout)) return r;
    if (int r = need_sorted_points(what, N)) return r;
    if ((uintptr_t)denc & 15) return tfail(-1, "field backward sorted pos: denc must be 16-byte aligned");
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int rows = backward_rows(N);
    hipLaunchKernelGGL(field_backward_pos_kernel<true>, dim3((unsigned)rows), dim3(kBwdThreads), 0, s, N,
                       backward_chunks(N), x, mask, (const float2*)grid, layout, w1, b1, w2, b2, color, dcolor, denc,
                       (float*)slab_scratch, dx);
    hipLaunchKernelGGL(slab_sum_kernel, grid_of(kMlpFloats, kSumCols), dim3(kSumCols * kSumGroups), 0, s, rows,
                       (const float*)slab_scratch, dw1, db1, dw2, db2);
    launch_sorted_dgrid(s, N, x, mask, denc, layout, dgrid, sort_scratch);
    return launched(what);
}

const char* gd_texture_last_error(void) { return gd::g_texture_err; }

}  // extern "C"
