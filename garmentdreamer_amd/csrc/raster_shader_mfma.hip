// raster_shader_mfma.hip -- the eight products of the neural shader on the bf16 matrix cores (C-ABI, layouts and rounding
// points: include/gd_shader.h; the fp32 side: raster_shader.hip), one launch per layer and kind, one tile kernel per kind:
//   forward          Y = bf16(act(X W^T + b))            rows_product_kernel<false>: X rows as A, W rows as B
//   input gradient   dZ_{l-1} = bf16([X > 0] dZ W)       rows_product_kernel<true>:  dZ rows as A, rows of W^T as B
//   weight gradient  dW = dZ^T X, db = dZ^T 1            points_product_kernel over slabs of points, then slab_sum_kernel
// All on v_mfma_f32_32x32x16_bf16.  Lane l (r = l & 31, h = l >> 5) holds A[row r][k = 8h + j] and B[k = 8h + j][col r],
// j = 0..7; accumulator register i of that lane is C[row (i & 3) + 8 (i >> 2) + 4h][col r].
//
// The two row products sum over the contiguous index of BOTH operands (X [n][k] with W [o][k]; dZ [n][o] with W^T [k][o]),
// so a fragment is one 16-byte global load and there is no LDS: a workgroup is 4 waves x 32 rows = the 128-row tile, 64
// columns wide, the packed weights (640 KB) stay in the L2.  The weight gradient sums over POINTS, the strided index of both
// operands: a chunk of 64 points x 64 columns of dZ and of X is written TRANSPOSED into two LDS images ([column][point],
// 128-byte rows with their 16-byte blocks permuted) and the fragments are 16-byte LDS reads.  No workgroup waits for another; no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_shader.h"
#include "nn_device.h"
#include "raster_common.h"
#include "raster_shader.h"

namespace gd {
namespace {

using gdnn::bf16x8_t;
using gdnn::f32x16;

struct Layer {
    int l, K, Kp, O, Op, relu;
};

Layer layer_of(int l)
{
    return Layer{l, gd_shader_in(l, 0), gd_shader_in(l, 1), gd_shader_out(l, 0), gd_shader_out(l, 1), gd_shader_relu(l)};
}

__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
__device__ __forceinline__ bool bf16_positive(uint16_t b) { return (b & 0x8000u) == 0 && (b & 0x7fffu) != 0; }

// C[128 rows from 128 blockIdx.x][64 columns from 64 blockIdx.y] = A [rows][depth] . B [columns][depth]^T, both bf16 with the
// summed index contiguous; `columns` is a multiple of 32.  BACKWARD = false, the forward of layer l: A = X_l, B = W_l,
// out = X_{l+1} with row stride ldo (logits for l = 7).  BACKWARD = true, its input gradient: A = dZ_l, B = W_l^T,
// out = dZ_{l-1} masked by x = X_l (none for l = 5, whose columns 256.. go to dextra; dfeat for l = 0).
template <bool BACKWARD>
__global__ __launch_bounds__(256) void rows_product_kernel(int l, int depth, int columns, int relu,
                                                           const int32_t* __restrict__ counters,
                                                           const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                                                           const float* __restrict__ bias, int bias_len,
                                                           const uint16_t* __restrict__ x, uint16_t* __restrict__ out, int ldo,
                                                           float* __restrict__ out32, float* __restrict__ dextra)
{
    const int64_t tile0 = (int64_t)blockIdx.x * GD_SHADER_TILE_ROWS;
    if (tile0 >= counters[0]) return;          // a tile at or past count: nothing to compute, nothing read
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t row0 = tile0 + 32 * wave;
    const int col0 = 64 * blockIdx.y;
    const bool second = col0 + 32 < columns;   // the last tile of 288 or 32 columns is 32 wide (wave-uniform)
    const uint16_t* a_ptr = A + (size_t)(row0 + r) * depth + 8 * h;
    const uint16_t* b0_ptr = B + (size_t)(col0 + r) * depth + 8 * h;
    const uint16_t* b1_ptr = b0_ptr + (size_t)32 * depth;
    f32x16 acc[2] = {};
    for (int k0 = 0; k0 < depth; k0 += 16) {
        const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(a_ptr + k0);
        const bf16x8_t b0 = *reinterpret_cast<const bf16x8_t*>(b0_ptr + k0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b0, acc[0], 0, 0, 0);
        if (second) {
            const bf16x8_t b1 = *reinterpret_cast<const bf16x8_t*>(b1_ptr + k0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b1, acc[1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; t++) {
        if (t == 1 && !second) break;
        const int col = col0 + 32 * t + r;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const size_t row = (size_t)(row0 + acc_row(i, h));
            float v = acc[t][i];
            if (!BACKWARD) {
                v = v + (col < bias_len ? bias[col] : 0.0f);
                if (l == 7) {
                    if (col < 3) out32[row * 3 + col] = v;
                } else {
                    out[row * ldo + col] = gdnn::f2bf(relu ? fmaxf(v, 0.0f) : v);
                }
            } else if (l == 0) {
                out32[row * 32 + col] = v;
            } else if (l == 5) {
                if (col < 256)
                    out[row * 256 + col] = gdnn::f2bf(v);
                else
                    dextra[row * 32 + (col - 256)] = v;
            } else {
                out[row * ldo + col] = gdnn::f2bf(bf16_positive(x[row * columns + col]) ? v : 0.0f);
            }
        }
    }
}

constexpr int kChunk = 64;        // points per LDS image: rows of 64 halves = 128 bytes = eight 16-byte blocks

// Half offset of (column c, point n) of a [64 columns][64 points] image.  The eight blocks of a row are permuted by
// (c ^ (c >> 3)) & 7: the 32 rows a fragment read touches spread over all eight block positions, and so do the eight
// columns 8 c' + j that the lanes of one transposed write touch.
__device__ __forceinline__ int image_at(int c, int n) { return c * kChunk + ((((n >> 3) ^ c ^ (c >> 3)) & 7) << 3) + (n & 7); }

// Slab blockIdx.y of layer l: partial[o][k] = sum over the slab's rows n of dZ[n][o] X[n][k] for the 64 x 64 tile
// blockIdx.x = to * tiles_k + tk, and partial_b[o] = sum of dZ[n][o] from the tiles with tk = 0.  Rows at or past the end of
// the last 128-row tile below count are not read; a slab that starts at or past count writes nothing and is not summed.
// A thread moves 8 columns of TWO consecutive points per chunk and writes them as eight 32-bit words (point 2p in the low
// half), so the transposition costs one LDS write per 2 x 1 elements and no sub-word write.
__global__ __launch_bounds__(256) void points_product_kernel(int Op, int Kp, int tiles_k, int64_t slab_rows,
                                                             const int32_t* __restrict__ counters,
                                                             const uint16_t* __restrict__ dz, const uint16_t* __restrict__ x,
                                                             float* __restrict__ partials)
{
    __shared__ __attribute__((aligned(16))) uint16_t zt[64 * kChunk];
    __shared__ __attribute__((aligned(16))) uint16_t xt[64 * kChunk];
    const int64_t count = counters[0];
    const int64_t begin = (int64_t)blockIdx.y * slab_rows;
    if (begin >= count) return;                // uniform over the workgroup, before any barrier
    const int64_t filled = (count + GD_SHADER_TILE_ROWS - 1) / GD_SHADER_TILE_ROWS * GD_SHADER_TILE_ROWS;
    const int64_t end = begin + slab_rows < filled ? begin + slab_rows : filled;
    const int o0 = 64 * (int)(blockIdx.x / tiles_k), k0 = 64 * (int)(blockIdx.x % tiles_k);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wo = wave & 1, wk = wave >> 1;
    const int pair = tid >> 3, c8 = (tid & 7) * 8;        // this thread moves 8 columns of the points 2 pair, 2 pair + 1
    const bool z_in = o0 + c8 < Op, x_in = k0 + c8 < Kp;
    const bool with_bias = k0 == 0 && wk == 0;
    bf16x8_t ones;
#pragma unroll
    for (int j = 0; j < 8; j++) ones[j] = (short)0x3f80;
    f32x16 acc = {}, acc_b = {};
    for (int64_t n0 = begin; n0 < end; n0 += kChunk) {
        gdnn::bf16x8 z0 = {}, z1 = {}, x0 = {}, x1 = {};
        if (z_in) {
            const uint16_t* src = dz + (size_t)(n0 + 2 * pair) * Op + o0 + c8;
            z0 = *reinterpret_cast<const gdnn::bf16x8*>(src);
            z1 = *reinterpret_cast<const gdnn::bf16x8*>(src + Op);
        }
        if (x_in) {
            const uint16_t* src = x + (size_t)(n0 + 2 * pair) * Kp + k0 + c8;
            x0 = *reinterpret_cast<const gdnn::bf16x8*>(src);
            x1 = *reinterpret_cast<const gdnn::bf16x8*>(src + Kp);
        }
        __syncthreads();                       // the fragments of the previous chunk have been read
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int at = image_at(c8 + j, 2 * pair);
            *reinterpret_cast<uint32_t*>(&zt[at]) = (uint32_t)z0.v[j] | ((uint32_t)z1.v[j] << 16);
            *reinterpret_cast<uint32_t*>(&xt[at]) = (uint32_t)x0.v[j] | ((uint32_t)x1.v[j] << 16);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kChunk / 16; s++) {
            const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(&zt[image_at(32 * wo + r, 16 * s + 8 * h)]);
            const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(&xt[image_at(32 * wk + r, 16 * s + 8 * h)]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
            if (with_bias) acc_b = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ones, acc_b, 0, 0, 0);
        }
    }
    float* partial = partials + (size_t)blockIdx.y * ((size_t)Op * Kp + Op);
    const int k = k0 + 32 * wk + r;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int o = o0 + 32 * wo + acc_row(i, h);
        if (o < Op && k < Kp) partial[(size_t)o * Kp + k] = acc[i];
        if (with_bias && r == 0 && o < Op) partial[(size_t)Op * Kp + o] = acc_b[i];
    }
}

// grad[o][k] += the slabs that start below count, in ascending order from 0; the same for the bias behind the weights
__global__ __launch_bounds__(256) void slab_sum_kernel(int O, int K, int Op, int Kp, int slabs, int64_t slab_rows,
                                                       const int32_t* __restrict__ counters, const float* __restrict__ partials,
                                                       float* __restrict__ dweight, float* __restrict__ dbias)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= O * K + O) return;
    const int64_t count = counters[0];
    const size_t stride = (size_t)Op * Kp + Op;
    const bool is_bias = e >= O * K;
    const size_t at = is_bias ? (size_t)Op * Kp + (e - O * K) : (size_t)(e / K) * Kp + (e % K);
    float sum = 0.0f;
    for (int s = 0; s < slabs && (int64_t)s * slab_rows < count; s++) sum += partials[(size_t)s * stride + at];
    float* dst = is_bias ? dbias + (e - O * K) : dweight + e;
    *dst += sum;
}

int layer_ok(const char* what, int l)
{
    if (l < 0 || l >= GD_SHADER_LAYERS) {
        char buf[200];
        snprintf(buf, sizeof(buf), "%s: the layer must be in [0, 7]", what);
        return mesh_fail(-1, buf);
    }
    return 0;
}

}  // namespace
}  // namespace gd

extern "C" {

int gd_shader_forward_layer(void* stream, int l, int64_t capacity, const int32_t* counters, const void* packed,
                            const float* params, void* act, float* logits)
{
    using namespace gd;
    if (layer_ok("shader forward", l) || shader_capacity_ok("shader forward", capacity)) return -1;
    if (!counters || !packed || !params || !act || (l == 7 && !logits)) return shader_null("shader forward");
    const Layer L = layer_of(l);
    const int64_t rows = gd_shader_rows(capacity);
    uint16_t* a = (uint16_t*)act;
    uint16_t* out = l == 7 ? nullptr : a + gd_shader_act_offset(l + 1, rows);
    const int ldo = l == 7 ? 0 : gd_shader_in(l + 1, 1);
    const dim3 grid((unsigned)(rows / GD_SHADER_TILE_ROWS), (unsigned)((L.Op + 63) / 64));
    hipLaunchKernelGGL(rows_product_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, l, L.Kp, L.Op, L.relu, counters,
                       (const uint16_t*)(a + gd_shader_act_offset(l, rows)),
                       (const uint16_t*)packed + gd_shader_packed_offset(l), params + gd_shader_param_offset(l, 1), L.O,
                       (const uint16_t*)nullptr, out, ldo, logits, (float*)nullptr);
    return mesh_launched(nullptr, "shader forward");
}

int gd_shader_backward_input_layer(void* stream, int l, int64_t capacity, const int32_t* counters, const void* packed_t,
                                   const void* act, void* dz, float* dfeat, float* dextra)
{
    using namespace gd;
    if (layer_ok("shader input gradient", l) || shader_capacity_ok("shader input gradient", capacity)) return -1;
    if (!counters || !packed_t || !act || !dz || (l == 0 && !dfeat) || (l == 5 && !dextra))
        return shader_null("shader input gradient");
    const Layer L = layer_of(l);
    const int64_t rows = gd_shader_rows(capacity);
    const uint16_t* a = (const uint16_t*)act;
    uint16_t* d = (uint16_t*)dz;
    uint16_t* out = l == 0 ? nullptr : d + gd_shader_dz_offset(l - 1, rows);
    const int ldo = l == 0 ? 0 : gd_shader_out(l - 1, 1);
    const dim3 grid((unsigned)(rows / GD_SHADER_TILE_ROWS), (unsigned)((L.Kp + 63) / 64));
    hipLaunchKernelGGL(rows_product_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, l, L.Op, L.Kp, 0, counters,
                       (const uint16_t*)(d + gd_shader_dz_offset(l, rows)),
                       (const uint16_t*)packed_t + gd_shader_packed_offset(l), (const float*)nullptr, 0,
                       a + gd_shader_act_offset(l, rows), out, ldo, dfeat, dextra);
    return mesh_launched(nullptr, "shader input gradient");
}

int gd_shader_backward_weight_layer(void* stream, int l, int64_t capacity, const int32_t* counters, const void* act,
                                    const void* dz, float* grad, void* scratch)
{
    using namespace gd;
    if (layer_ok("shader weight gradient", l) || shader_capacity_ok("shader weight gradient", capacity)) return -1;
    if (!counters || !act || !dz || !grad || !scratch) return shader_null("shader weight gradient");
    const Layer L = layer_of(l);
    const int64_t rows = gd_shader_rows(capacity);
    const int64_t S = gd_shader_slab_rows(rows);
    const int slabs = (int)((rows + S - 1) / S);
    float* partials = (float*)((char*)scratch + shader_l1_scratch_bytes(rows));
    const int tiles_o = (L.Op + 63) / 64, tiles_k = (L.Kp + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(points_product_kernel, dim3((unsigned)(tiles_o * tiles_k), (unsigned)slabs), dim3(256), 0, st, L.Op, L.Kp,
                       tiles_k, S, counters, (const uint16_t*)dz + gd_shader_dz_offset(l, rows),
                       (const uint16_t*)act + gd_shader_act_offset(l, rows), partials);
    hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)((L.O * L.K + L.O + 255) / 256)), dim3(256), 0, st, L.O, L.K, L.Op, L.Kp,
                       slabs, S, counters, (const float*)partials, grad + gd_shader_param_offset(l, 0),
                       grad + gd_shader_param_offset(l, 1));
    return mesh_launched(nullptr, "shader weight gradient");
}

}  // extern "C"
