// raster_shader.hip -- the fp32 element-wise side of the neural shader and the shading loss of the deformer's second stage
// (C-ABI, layouts and the DEFINITIONS: include/gd_shader.h): selection, features, pack, L1 and feature backward.  Built with
// -ffp-contract=off: the header fixes the order of every operation.  The eight products are in raster_shader_mfma.hip.
//
// Nothing here is tuned: every kernel is one thread per pixel or per point over a few dozen bytes.  What the file is for is
// the missing host round trip (the reference gathers by a boolean mask and draws a host randperm) and fixed-order sums.
//   selection  select_count_kernel (ballots per 256 pixels) -> select_scan_kernel (ONE workgroup walks the counts in chunks
//              of 256) -> select_scatter_kernel (each workgroup repeats its ballots); no workgroup waits for another
//   L1         l1_rows_kernel (LDS tree per 256 rows) -> l1_final_kernel (one workgroup), the sums of gd_mesh_losses.h
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_shader.h"
#include "nn_device.h"
#include "raster_mesh_common.h"
#include "raster_shader.h"

namespace gd {
namespace {

constexpr float kViewEps = 1e-6f;     // the eps the reference passes for every cosine with the view direction

struct Selection {
    const float *normal, *position, *mask, *view_mask, *camera;
    uint32_t seed, step, threshold;
    int all;   // p >= 1
};

// SELECTION of gd_shader.h for pixel i
__device__ __forceinline__ bool kept(const Selection& s, size_t i)
{
    if (!(s.view_mask[i] > 0.0f && s.mask[i] > 0.0f)) return false;
    const Camera cam = load_camera(s.camera);
    const V3 n_cam = to_camera(cam, load3(s.normal, i));
    V3 u;
    float l;
    const V3 d = view_direction(cam, load3(s.position, i), &u, &l);
    if (!(cosine(d, n_cam, kViewEps) <= 0.0f)) return false;
    return s.all || gd_shader_hash32(s.seed, s.step, (uint32_t)i) < s.threshold;
}

// exclusive prefix of `flag` over the workgroup's 256 threads in thread order; *total receives the workgroup's sum
__device__ __forceinline__ int block_flag_scan(bool flag, int* lds4, int* total)
{
    const unsigned long long ballot = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int before = __popcll(ballot & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) lds4[wave] = __popcll(ballot);
    __syncthreads();
    int base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const int c = lds4[w];
        if (w < wave) base += c;
        sum += c;
    }
    *total = sum;
    return base + before;
}

__global__ __launch_bounds__(256) void select_count_kernel(size_t npix, Selection s, int* __restrict__ counts)
{
    __shared__ int lds4[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int total;
    block_flag_scan(i < npix && kept(s, i), lds4, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// ONE workgroup: offsets[b] = sum of counts[0 .. b - 1]; counters = {count, dropped, kept, 0}
__global__ __launch_bounds__(256) void select_scan_kernel(int blocks, const int* __restrict__ counts, int* __restrict__ offsets,
                                                          int64_t capacity, int32_t* __restrict__ counters)
{
    __shared__ int lds[256];
    const int t = threadIdx.x;
    int base = 0;
    for (int c = 0; c < blocks; c += 256) {
        const int v = c + t < blocks ? counts[c + t] : 0;
        lds[t] = v;
        __syncthreads();
        for (int stride = 1; stride < 256; stride <<= 1) {   // inclusive scan, every thread passes every barrier
            const int add = t >= stride ? lds[t - stride] : 0;
            __syncthreads();
            lds[t] += add;
            __syncthreads();
        }
        if (c + t < blocks) offsets[c + t] = base + lds[t] - v;
        base += lds[255];
        __syncthreads();
    }
    if (t == 0) {
        const int count = (int64_t)base < capacity ? base : (int)capacity;
        counters[0] = count;
        counters[1] = base - count;
        counters[2] = base;
        counters[3] = 0;
    }
}

__global__ __launch_bounds__(256) void select_scatter_kernel(size_t npix, Selection s, const int* __restrict__ offsets,
                                                             int64_t capacity, int32_t* __restrict__ index)
{
    __shared__ int lds4[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool flag = i < npix && kept(s, i);
    int total;
    const int64_t pos = (int64_t)offsets[blockIdx.x] + block_flag_scan(flag, lds4, &total);
    if (flag && pos < capacity) index[pos] = (int32_t)i;
}

// ---- features ---------------------------------------------------------------------------------------------------------

struct alignas(16) Row32 {
    uint16_t v[32];
};

__device__ __forceinline__ void store_row32(uint16_t* __restrict__ dst, const Row32& r)
{
    const uint4* src = reinterpret_cast<const uint4*>(r.v);
    uint4* d = reinterpret_cast<uint4*>(dst);
#pragma unroll
    for (int k = 0; k < 4; k++) d[k] = src[k];
}

// feat and extra of one point, rounded, into row r of X_0 and the extra columns of X_5
__device__ __forceinline__ void write_features(uint16_t* __restrict__ x0, uint16_t* __restrict__ x5, int64_t r, V3 p, V3 n, V3 u)
{
    Row32 feat = {}, extra = {};
    const float pc[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int c = 0; c < 3; c++) feat.v[c] = gdnn::f2bf(pc[c]);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float f = (float)(1 << j);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float a = f * pc[c];
            feat.v[3 + 6 * j + c] = gdnn::f2bf(sinf(a));
            feat.v[6 + 6 * j + c] = gdnn::f2bf(cosf(a));
        }
    }
    extra.v[0] = gdnn::f2bf(n.x);
    extra.v[1] = gdnn::f2bf(n.y);
    extra.v[2] = gdnn::f2bf(n.z);
    extra.v[3] = gdnn::f2bf(u.x);
    extra.v[4] = gdnn::f2bf(u.y);
    extra.v[5] = gdnn::f2bf(u.z);
    store_row32(x0 + r * 32, feat);
    store_row32(x5 + r * 288 + 256, extra);
}

__device__ __forceinline__ void write_zero_features(uint16_t* __restrict__ x0, uint16_t* __restrict__ x5, int64_t r)
{
    const Row32 zero = {};
    store_row32(x0 + r * 32, zero);
    store_row32(x5 + r * 288 + 256, zero);
}

__global__ __launch_bounds__(256) void features_kernel(int64_t rows, const float* __restrict__ position,
                                                       const float* __restrict__ normal, const float* __restrict__ camera,
                                                       const int32_t* __restrict__ index, const int32_t* __restrict__ counters,
                                                       uint16_t* __restrict__ x0, uint16_t* __restrict__ x5)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    if (r >= counters[0]) {
        write_zero_features(x0, x5, r);
        return;
    }
    const size_t i = (size_t)index[r];
    const V3 p = load3(position, i);
    float l;
    const V3 u = unit_to_center(load3(camera, 3), p, &l);
    write_features(x0, x5, r, p, load3(normal, i), u);
}

__global__ __launch_bounds__(256) void features_points_kernel(int64_t rows, int64_t N, const float* __restrict__ position,
                                                              const float* __restrict__ normal,
                                                              const float* __restrict__ view_dir, int32_t* __restrict__ counters,
                                                              uint16_t* __restrict__ x0, uint16_t* __restrict__ x5)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r == 0) {
        counters[0] = (int32_t)N;
        counters[1] = 0;
        counters[2] = (int32_t)N;
        counters[3] = 0;
    }
    if (r >= rows) return;
    if (r >= N)
        write_zero_features(x0, x5, r);
    else
        write_features(x0, x5, r, load3(position, (size_t)r), load3(normal, (size_t)r), load3(view_dir, (size_t)r));
}

// ---- pack -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ params, uint16_t* __restrict__ packed,
                                                   uint16_t* __restrict__ packed_t)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= GD_SHADER_PACKED_ELEMS) return;
    int l = 0;
    while (e >= gd_shader_packed_offset(l + 1)) l++;
    const size_t off = gd_shader_packed_offset(l);
    const int Kp = gd_shader_in(l, 1), Op = gd_shader_out(l, 1), K = gd_shader_in(l, 0), O = gd_shader_out(l, 0);
    const int o = (int)((e - off) / Kp), k = (int)((e - off) % Kp);
    const uint16_t w = o < O && k < K ? gdnn::f2bf(params[gd_shader_param_offset(l, 0) + (size_t)o * K + k]) : (uint16_t)0;
    packed[e] = w;
    packed_t[off + (size_t)k * Op + o] = w;
}

// ---- L1 ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float sigmoid(float logit) { return 1.0f / (1.0f + expf(-logit)); }

__global__ __launch_bounds__(256) void l1_rows_kernel(const int32_t* __restrict__ index, const int32_t* __restrict__ counters,
                                                      const float* __restrict__ logits, const float* __restrict__ rgb,
                                                      float* __restrict__ partials)
{
    __shared__ float lds[256];
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float term = 0.0f;
    if (r < counters[0]) {
        const V3 z = load3(logits, (size_t)r), t = load3(rgb, (size_t)index[r]);
        term = (fabsf(sigmoid(z.x) - t.x) + fabsf(sigmoid(z.y) - t.y)) + fabsf(sigmoid(z.z) - t.z);
    }
    const float total = block_tree_sum(term, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void l1_final_kernel(int blocks, const float* __restrict__ partials,
                                                       const int32_t* __restrict__ counters, float* __restrict__ loss)
{
    __shared__ float lds[256];
    float x = 0.0f;
    for (int b = threadIdx.x; b < blocks; b += 256) x += partials[b];
    const float sum = block_tree_sum(x, lds);
    const int count = counters[0];
    if (threadIdx.x == 0) loss[0] = count > 0 ? sum / (3.0f * (float)count) : 0.0f;
}

__device__ __forceinline__ float l1_gradient(float logit, float target, float k)
{
    const float c = sigmoid(logit);
    const float g = k * (c * (1.0f - c));
    return c > target ? g : (c < target ? -g : 0.0f);
}

__global__ __launch_bounds__(256) void l1_backward_kernel(int64_t rows, const int32_t* __restrict__ index,
                                                          const int32_t* __restrict__ counters, const float* __restrict__ logits,
                                                          const float* __restrict__ rgb, const float* __restrict__ dloss,
                                                          uint16_t* __restrict__ dz7, float* __restrict__ dlogits)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    Row32 out = {};
    V3 g = V3{0.0f, 0.0f, 0.0f};
    const int count = counters[0];
    if (r < count) {
        const float k = dloss[0] / (3.0f * (float)count);
        const V3 z = load3(logits, (size_t)r), t = load3(rgb, (size_t)index[r]);
        g = V3{l1_gradient(z.x, t.x, k), l1_gradient(z.y, t.y, k), l1_gradient(z.z, t.z, k)};
        out.v[0] = gdnn::f2bf(g.x);
        out.v[1] = gdnn::f2bf(g.y);
        out.v[2] = gdnn::f2bf(g.z);
    }
    store_row32(dz7 + r * 32, out);
    if (dlogits) store3(dlogits, (size_t)r, g);
}

__global__ __launch_bounds__(256) void colour_kernel(int64_t n, const float* __restrict__ logits, float* __restrict__ colour)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) colour[e] = sigmoid(logits[e]);
}

// ---- feature backward ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void features_backward_kernel(int64_t rows, const float* __restrict__ position,
                                                                const float* __restrict__ camera,
                                                                const int32_t* __restrict__ index,
                                                                const int32_t* __restrict__ counters,
                                                                const float* __restrict__ dfeat, const float* __restrict__ dextra,
                                                                float* __restrict__ dposition, float* __restrict__ dnormal)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows || r >= counters[0]) return;
    const size_t i = (size_t)index[r];
    const V3 p = load3(position, i);
    const float* df = dfeat + r * 32;
    const float* de = dextra + r * 32;
    const float pc[3] = {p.x, p.y, p.z};
    float dp[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float acc = df[c];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float f = (float)(1 << j);
            const float a = f * pc[c];
            acc = acc + f * (cosf(a) * df[3 + 6 * j + c] - sinf(a) * df[6 + 6 * j + c]);
        }
        dp[c] = acc;
    }
    float l;
    const V3 u = unit_to_center(load3(camera, 3), p, &l);
    const V3 gu = V3{de[3], de[4], de[5]};
    const V3 gv = l > kNormEps ? divide(sub(gu, scale(u, dot(u, gu))), l) : divide(gu, kNormEps);
    store3(dposition, i, V3{dp[0] - gv.x, dp[1] - gv.y, dp[2] - gv.z});
    store3(dnormal, i, V3{de[0], de[1], de[2]});
}

int image_ok(const char* what, int H, int W)
{
    if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 30)) {
        char buf[200];
        snprintf(buf, sizeof(buf), "%s: H and W must be positive and H W < 2^30", what);
        return mesh_fail(-1, buf);
    }
    return 0;
}

}  // namespace

int shader_capacity_ok(const char* what, int64_t capacity)
{
    if (capacity < 1 || capacity > ((int64_t)1 << 24)) {
        char buf[200];
        snprintf(buf, sizeof(buf), "%s: capacity must be in [1, 2^24]", what);
        return mesh_fail(-1, buf);
    }
    return 0;
}

int shader_null(const char* what)
{
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: null pointer", what);
    return mesh_fail(-1, buf);
}

size_t shader_align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace gd

extern "C" {

size_t gd_shader_select_scratch_bytes(int64_t pixels)
{
    if (pixels <= 0) return 0;
    return gd::shader_align256(((size_t)pixels + 255) / 256 * 2 * sizeof(int));
}

size_t gd_shader_scratch_bytes(int64_t capacity)
{
    if (capacity < 1 || capacity > ((int64_t)1 << 24)) return 0;
    const int64_t rows = gd_shader_rows(capacity);
    const int64_t S = gd_shader_slab_rows(rows);
    const size_t slabs = (size_t)((rows + S - 1) / S);
    return gd::shader_l1_scratch_bytes(rows) + gd::shader_align256(slabs * gd::kShaderSlabFloats * sizeof(float));
}

int gd_shader_select(void* stream, int H, int W, const float* normal, const float* position, const float* mask,
                     const float* view_mask, const float* camera, float p, uint32_t seed, uint32_t step, int64_t capacity,
                     int32_t* index, int32_t* counters, void* scratch)
{
    using namespace gd;
    if (image_ok("shader select", H, W) || shader_capacity_ok("shader select", capacity)) return -1;
    if (!(p >= 0.0f)) return mesh_fail(-1, "shader select: p must not be negative");
    if (!normal || !position || !mask || !view_mask || !camera || !index || !counters || !scratch)
        return shader_null("shader select");
    const size_t npix = (size_t)H * W;
    const unsigned blocks = (unsigned)((npix + 255) / 256);
    const bool all = p >= 1.0f;
    const Selection s = {normal, position, mask, view_mask, camera, seed, step, all ? 0u : gd_shader_keep_threshold(p), all};
    int* counts = (int*)scratch;
    int* offsets = counts + blocks;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(select_count_kernel, dim3(blocks), dim3(256), 0, st, npix, s, counts);
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, st, (int)blocks, (const int*)counts, offsets, capacity, counters);
    hipLaunchKernelGGL(select_scatter_kernel, dim3(blocks), dim3(256), 0, st, npix, s, (const int*)offsets, capacity, index);
    return mesh_launched(nullptr, "shader select");
}

int gd_shader_features(void* stream, int H, int W, const float* position, const float* normal, const float* camera,
                       int64_t capacity, const int32_t* index, const int32_t* counters, void* act)
{
    using namespace gd;
    if (image_ok("shader features", H, W) || shader_capacity_ok("shader features", capacity)) return -1;
    if (!position || !normal || !camera || !index || !counters || !act) return shader_null("shader features");
    const int64_t rows = gd_shader_rows(capacity);
    uint16_t* a = (uint16_t*)act;
    hipLaunchKernelGGL(features_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, position,
                       normal, camera, index, counters, a + gd_shader_act_offset(0, rows), a + gd_shader_act_offset(5, rows));
    return mesh_launched(nullptr, "shader features");
}

int gd_shader_features_points(void* stream, int64_t N, const float* position, const float* normal, const float* view_dir,
                              int64_t capacity, int32_t* counters, void* act)
{
    using namespace gd;
    if (shader_capacity_ok("shader features of points", capacity)) return -1;
    if (N < 1 || N > capacity) return mesh_fail(-1, "shader features of points: N must be in [1, capacity]");
    if (!position || !normal || !view_dir || !counters || !act) return shader_null("shader features of points");
    const int64_t rows = gd_shader_rows(capacity);
    uint16_t* a = (uint16_t*)act;
    hipLaunchKernelGGL(features_points_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, N,
                       position, normal, view_dir, counters, a + gd_shader_act_offset(0, rows),
                       a + gd_shader_act_offset(5, rows));
    return mesh_launched(nullptr, "shader features of points");
}

int gd_shader_pack(void* stream, const float* params, void* packed, void* packed_t)
{
    using namespace gd;
    if (!params || !packed || !packed_t) return shader_null("shader pack");
    hipLaunchKernelGGL(pack_kernel, dim3(GD_SHADER_PACKED_ELEMS / 256), dim3(256), 0, (hipStream_t)stream, params,
                       (uint16_t*)packed, (uint16_t*)packed_t);
    return mesh_launched(nullptr, "shader pack");
}

int gd_shader_l1_forward(void* stream, int H, int W, int64_t capacity, const int32_t* index, const int32_t* counters,
                         const float* logits, const float* rgb, float* loss, void* scratch)
{
    using namespace gd;
    if (image_ok("shader L1", H, W) || shader_capacity_ok("shader L1", capacity)) return -1;
    if (!index || !counters || !logits || !rgb || !loss || !scratch) return shader_null("shader L1");
    const int64_t rows = gd_shader_rows(capacity);
    const unsigned blocks = (unsigned)((rows + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(l1_rows_kernel, dim3(blocks), dim3(256), 0, st, index, counters, logits, rgb, (float*)scratch);
    hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(256), 0, st, (int)blocks, (const float*)scratch, counters, loss);
    return mesh_launched(nullptr, "shader L1");
}

int gd_shader_l1_backward(void* stream, int H, int W, int64_t capacity, const int32_t* index, const int32_t* counters,
                          const float* logits, const float* rgb, const float* dloss, void* dz, float* dlogits)
{
    using namespace gd;
    if (image_ok("shader L1 backward", H, W) || shader_capacity_ok("shader L1 backward", capacity)) return -1;
    if (!index || !counters || !logits || !rgb || !dloss || !dz) return shader_null("shader L1 backward");
    const int64_t rows = gd_shader_rows(capacity);
    hipLaunchKernelGGL(l1_backward_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, index,
                       counters, logits, rgb, dloss, (uint16_t*)dz + gd_shader_dz_offset(7, rows), dlogits);
    return mesh_launched(nullptr, "shader L1 backward");
}

int gd_shader_colour(void* stream, int64_t N, const float* logits, float* colour)
{
    using namespace gd;
    if (N < 1 || N > ((int64_t)1 << 24)) return mesh_fail(-1, "shader colour: N must be in [1, 2^24]");
    if (!logits || !colour) return shader_null("shader colour");
    hipLaunchKernelGGL(colour_kernel, dim3((unsigned)((3 * N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, 3 * N, logits,
                       colour);
    return mesh_launched(nullptr, "shader colour");
}

int gd_shader_features_backward(void* stream, int H, int W, const float* position, const float* camera, int64_t capacity,
                                const int32_t* index, const int32_t* counters, const float* dfeat, const float* dextra,
                                float* dposition, float* dnormal)
{
    using namespace gd;
    if (image_ok("shader features backward", H, W) || shader_capacity_ok("shader features backward", capacity)) return -1;
    if (!position || !camera || !index || !counters || !dfeat || !dextra || !dposition || !dnormal)
        return shader_null("shader features backward");
    const int64_t rows = gd_shader_rows(capacity);
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)H * W * 3 * sizeof(float);
    if (hipMemsetAsync(dposition, 0, bytes, st) != hipSuccess || hipMemsetAsync(dnormal, 0, bytes, st) != hipSuccess)
        return mesh_launched(nullptr, "shader features backward");
    hipLaunchKernelGGL(features_backward_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, rows, position, camera,
                       index, counters, dfeat, dextra, dposition, dnormal);
    return mesh_launched(nullptr, "shader features backward");
}

}  // extern "C"
