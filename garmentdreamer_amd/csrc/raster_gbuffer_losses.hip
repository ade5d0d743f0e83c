// raster_gbuffer_losses.hip -- the G-buffer losses of the mesh deformer's second stage (C-ABI and the DEFINITIONS:
// include/gd_mesh_losses.h): the enhanced and the plain normal-map loss and the hole-mask loss of one view, forward and
// backward (Garment_Deformer_NeTF/deformer/losses/normal.py, losses/mask.py).  Built with -ffp-contract=off: the header
// fixes the order of every operation.
//
// Bandwidth-trivial (seven floats per pixel and buffer set): one thread per pixel, plain loads, nothing tuned.  What the
// file is for is the launch count (the torch composition is some thirty elementwise launches per term and view), the
// missing host synchronisation (the composition ends in a boolean-mask gather) and the contract of raster_geometry.hip: no
// floating-point atomics, so reruns are bit-identical.
//   forward    losses_pixel_kernel (thread per pixel; six LDS trees into partials) -> losses_final_kernel (one workgroup)
//   backward   losses_backward_kernel (thread per pixel, recomputes the terms; reads Z and the counts from stats)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_mesh_losses.h"
#include "raster_mesh_common.h"

namespace gd {
namespace {

constexpr float kErrEps = 1e-8f;      // cosine_similarity's default, the enhanced loss's error term
constexpr float kViewEps = 1e-6f;     // the eps the reference passes for every cosine with the view direction
constexpr int kSums = 6;              // e w, w, plain, hole (float); plain in, hole in (int32)

// R^T h
__device__ __forceinline__ V3 transposed(const Camera& c, V3 h)
{
    return V3{(c.row[0].x * h.x + c.row[1].x * h.y) + c.row[2].x * h.z,
              (c.row[0].y * h.x + c.row[1].y * h.y) + c.row[2].y * h.z,
              (c.row[0].z * h.x + c.row[1].z * h.y) + c.row[2].z * h.z};
}

// B(g) = R^T (g_0, -g_1, -g_2)
__device__ __forceinline__ V3 to_world(const Camera& c, V3 g) { return transposed(c, V3{g.x, -g.y, -g.z}); }

// C_e(a, b): the adjoint of cos_e(a, b) towards b
__device__ __forceinline__ V3 cosine_adjoint(V3 a, V3 b, float eps)
{
    const float la = norm(a), lb = norm(b);
    const float ma = fmaxf(la, eps), mb = fmaxf(lb, eps);
    V3 D = divide(a, ma);
    if (lb > eps) D = sub(D, divide(scale(b, dot(a, b) / (ma * mb)), mb));
    return divide(D, mb);
}

__device__ __forceinline__ float sign_of(float c) { return c < 0.0f ? -1.0f : 1.0f; }

// the per-pixel quantities both passes need
struct Pixel {
    V3 n_cam, d, u, T, t;
    float l;
    float e, w;           // enhanced
    V3 diff;              // plain
    float ds;             // hole: s - s_rf
    bool in_enhanced, in_plain, in_hole;
};

struct Inputs {
    const float *normal, *position, *mask, *normal_rf, *position_rf, *mask_rf, *target_normal, *target_mask;
};

__device__ __forceinline__ Pixel pixel_terms(const Inputs& in, const Camera& cam, int terms, float epsilon, size_t i)
{
    Pixel px = {};
    const float m = in.mask[i];
    px.n_cam = to_camera(cam, load3(in.normal, i));
    if (terms & (GD_MESH_LOSSES_ENHANCED | GD_MESH_LOSSES_HOLE))
        px.d = view_direction(cam, load3(in.position, i), &px.u, &px.l);
    float tm = 0.0f;
    if (terms & (GD_MESH_LOSSES_ENHANCED | GD_MESH_LOSSES_PLAIN)) {
        px.T = load3(in.target_normal, i);
        tm = in.target_mask[i];
    }
    if (terms & GD_MESH_LOSSES_ENHANCED) {
        px.t = V3{2.0f * px.T.x - 1.0f, 2.0f * px.T.y - 1.0f, 2.0f * px.T.z - 1.0f};
        px.e = 1.0f - cosine(px.t, px.n_cam, kErrEps);
        float ct = cosine(px.d, px.t, kViewEps);
        if (ct > epsilon) ct = 0.0f;
        const float cv = cosine(px.d, px.n_cam, kViewEps);
        px.w = expf(fabsf(ct));
        px.in_enhanced = tm > 0.0f && m > 0.0f && cv <= 0.0f && ct <= epsilon;
    }
    if (terms & GD_MESH_LOSSES_PLAIN) {
        px.diff = V3{0.5f * (px.n_cam.x + 1.0f) - px.T.x, 0.5f * (px.n_cam.y + 1.0f) - px.T.y,
                     0.5f * (px.n_cam.z + 1.0f) - px.T.z};
        px.in_plain = tm > 0.0f && m > 0.0f;
    }
    if (terms & GD_MESH_LOSSES_HOLE) {
        V3 u_rf;
        float l_rf;
        const V3 d_rf = view_direction(cam, load3(in.position_rf, i), &u_rf, &l_rf);
        const V3 n_rf = to_camera(cam, load3(in.normal_rf, i));
        px.ds = sign_of(cosine(px.d, px.n_cam, kViewEps)) - sign_of(cosine(d_rf, n_rf, kViewEps));
        px.in_hole = m > 0.0f && in.mask_rf[i] > 0.0f;
    }
    return px;
}

// partials: [kSums][blocks] words, rows 0..3 float, rows 4..5 int32
__global__ __launch_bounds__(256) void losses_pixel_kernel(size_t npix, int terms, Inputs in,
                                                           const float* __restrict__ camera, float epsilon,
                                                           float* __restrict__ partials)
{
    __shared__ float lds_f[4][256];
    __shared__ int lds_i[2][256];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    float f[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int c[2] = {0, 0};
    if (i < npix) {
        const Camera cam = load_camera(camera);
        const Pixel px = pixel_terms(in, cam, terms, epsilon, i);
        if (terms & GD_MESH_LOSSES_ENHANCED) {
            f[1] = px.w;
            if (px.in_enhanced) f[0] = px.e * px.w;
        }
        if (px.in_plain) {
            f[2] = (fabsf(px.diff.x) + fabsf(px.diff.y)) + fabsf(px.diff.z);
            c[0] = 1;
        }
        if (px.in_hole) {
            f[3] = px.ds * px.ds;
            c[1] = 1;
        }
    }
    const size_t blocks = gridDim.x;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float total = block_tree_sum(f[k], lds_f[k]);
        if (threadIdx.x == 0) partials[k * blocks + blockIdx.x] = total;
    }
    int* counts = reinterpret_cast<int*>(partials);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int total = block_tree_sum(c[k], lds_i[k]);
        if (threadIdx.x == 0) counts[(4 + k) * blocks + blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(256) void losses_final_kernel(int blocks, const float* __restrict__ partials,
                                                           float* __restrict__ stats)
{
    __shared__ float lds_f[4][256];
    __shared__ int lds_i[2][256];
    const int* counts = reinterpret_cast<const int*>(partials);
    float f[4];
    int c[2];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float x = 0.0f;
        for (int b = threadIdx.x; b < blocks; b += 256) x += partials[(size_t)k * blocks + b];
        f[k] = block_tree_sum(x, lds_f[k]);
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
        int x = 0;
        for (int b = threadIdx.x; b < blocks; b += 256) x += counts[(size_t)(4 + k) * blocks + b];
        c[k] = block_tree_sum(x, lds_i[k]);
    }
    if (threadIdx.x == 0) {
        stats[0] = f[1] > 0.0f ? f[0] / f[1] : 0.0f;
        stats[1] = c[0] > 0 ? f[2] / (3.0f * (float)c[0]) : 0.0f;
        stats[2] = c[1] > 0 ? f[3] / (float)c[1] : 0.0f;
        stats[3] = f[1];
        int* out = reinterpret_cast<int*>(stats);
        out[4] = c[0];
        out[5] = c[1];
    }
}

__global__ __launch_bounds__(256) void losses_backward_kernel(size_t npix, int terms, Inputs in,
                                                              const float* __restrict__ camera, float epsilon,
                                                              const float* __restrict__ stats,
                                                              const float* __restrict__ dloss,
                                                              float* __restrict__ dnormal, float* __restrict__ dposition)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const Camera cam = load_camera(camera);
    const Pixel px = pixel_terms(in, cam, terms, epsilon, i);
    const float Z = stats[3];
    const int* counts = reinterpret_cast<const int*>(stats);
    const int count_plain = counts[4], count_hole = counts[5];
    V3 g = V3{0.0f, 0.0f, 0.0f}, dp = V3{0.0f, 0.0f, 0.0f};
    if (px.in_enhanced && Z > 0.0f)
        g = add(g, scale(cosine_adjoint(px.t, px.n_cam, kErrEps), -(dloss[0] * (px.w / Z))));
    if (px.in_plain && count_plain > 0) {
        const float k = dloss[1] * (0.5f / (3.0f * (float)count_plain));
        const V3 s = V3{px.diff.x > 0.0f ? k : (px.diff.x < 0.0f ? -k : 0.0f),
                        px.diff.y > 0.0f ? k : (px.diff.y < 0.0f ? -k : 0.0f),
                        px.diff.z > 0.0f ? k : (px.diff.z < 0.0f ? -k : 0.0f)};
        g = add(g, s);
    }
    if (px.in_hole && count_hole > 0) {
        const float k = dloss[2] * (2.0f * px.ds / (float)count_hole);
        g = add(g, scale(cosine_adjoint(px.d, px.n_cam, kViewEps), k));
        const V3 gd = scale(cosine_adjoint(px.n_cam, px.d, kViewEps), k);
        const V3 gu = transposed(cam, V3{-gd.x, gd.y, gd.z});
        const V3 gv = px.l > kNormEps ? divide(sub(gu, scale(px.u, dot(px.u, gu))), px.l) : divide(gu, kNormEps);
        dp = V3{-gv.x, -gv.y, -gv.z};
    }
    store3(dnormal, i, to_world(cam, g));
    store3(dposition, i, dp);
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// -1 with a message, or 0: what both entries check before any device work
int validate(const char* what, int H, int W, int terms, const Inputs& in, const float* camera)
{
    char buf[200];
    if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 30)) {
        snprintf(buf, sizeof(buf), "%s: H and W must be positive and H W < 2^30", what);
        return mesh_fail(-1, buf);
    }
    if (terms <= 0 || (terms & ~GD_MESH_LOSSES_ALL)) {
        snprintf(buf, sizeof(buf), "%s: terms must be a non-empty subset of ENHANCED | PLAIN | HOLE", what);
        return mesh_fail(-1, buf);
    }
    const bool rf = terms & GD_MESH_LOSSES_HOLE, target = terms & (GD_MESH_LOSSES_ENHANCED | GD_MESH_LOSSES_PLAIN);
    if (!in.normal || !in.position || !in.mask || !camera || (rf && (!in.normal_rf || !in.position_rf || !in.mask_rf))
        || (target && (!in.target_normal || !in.target_mask))) {
        snprintf(buf, sizeof(buf), "%s: null pointer", what);
        return mesh_fail(-1, buf);
    }
    return 0;
}

}  // namespace
}  // namespace gd

extern "C" {

size_t gd_mesh_gbuffer_losses_scratch_bytes(int64_t pixels)
{
    if (pixels <= 0) return 0;
    return gd::align256(((size_t)pixels + 255) / 256 * gd::kSums * sizeof(float));
}

int gd_mesh_gbuffer_losses_forward(void* stream, int H, int W, int terms, const float* normal, const float* position,
                                   const float* mask, const float* normal_rf, const float* position_rf,
                                   const float* mask_rf, const float* target_normal, const float* target_mask,
                                   const float* camera, float epsilon, void* stats, void* scratch)
{
    using namespace gd;
    const Inputs in = {normal, position, mask, normal_rf, position_rf, mask_rf, target_normal, target_mask};
    if (validate("gbuffer losses", H, W, terms, in, camera)) return -1;
    if (!stats || !scratch) return mesh_fail(-1, "gbuffer losses: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const size_t npix = (size_t)H * W;
    const unsigned blocks = (unsigned)((npix + 255) / 256);
    hipLaunchKernelGGL(losses_pixel_kernel, dim3(blocks), dim3(256), 0, s, npix, terms, in, camera, epsilon,
                       (float*)scratch);
    hipLaunchKernelGGL(losses_final_kernel, dim3(1), dim3(256), 0, s, (int)blocks, (const float*)scratch, (float*)stats);
    return mesh_launched(nullptr, "gbuffer losses forward");
}

int gd_mesh_gbuffer_losses_backward(void* stream, int H, int W, int terms, const float* normal, const float* position,
                                    const float* mask, const float* normal_rf, const float* position_rf,
                                    const float* mask_rf, const float* target_normal, const float* target_mask,
                                    const float* camera, float epsilon, const void* stats, const float* dloss,
                                    float* dnormal, float* dposition)
{
    using namespace gd;
    const Inputs in = {normal, position, mask, normal_rf, position_rf, mask_rf, target_normal, target_mask};
    if (validate("gbuffer losses backward", H, W, terms, in, camera)) return -1;
    if (!stats || !dloss || !dnormal || !dposition) return mesh_fail(-1, "gbuffer losses backward: null pointer");
    const size_t npix = (size_t)H * W;
    hipLaunchKernelGGL(losses_backward_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       npix, terms, in, camera, epsilon, (const float*)stats, dloss, dnormal, dposition);
    return mesh_launched(nullptr, "gbuffer losses backward");
}

}  // extern "C"
